#!/usr/bin/env python3
"""What the exact diagonal of the Gauss-Newton Hessian costs with the forward fields in HBM, at config 4's survey: bench.py's 512^2 Marmousi-like model
(dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr.  Prints one JSON object and writes it to --out (default
profiles/gaussnewton_bench.json).

Routes.  One problem with an explicit density (Gardner's formula evaluated once), its store F = fieldsDevice() and the factors of A and A^T resident.  After a
warm-up of each, the calls alternate one by one, `reps` rounds: illumination(u=F, kind='gaussNewton') and illumination(u=F) (the pseudo-Hessian) per
linearisation, and Jtvec(u=F, adjoint='transpose', linearisation='full') of the same run, the yardstick: the new call solves nrec columns per frequency through
A^-T where Jtvec solves nsrc, then streams the store once.

Kernels, on an assembled n^2 handle and nsrc random columns (wall time around the call, launch and stream synchronisation included; `empty_call` is that
overhead alone, the same entry point on a 3 x 3 handle):

  copy_c128                        a device-to-device copy of the complex128 columns, the rate everything is compared with
  lag_gram_c128 / lag_gram_c64     k_lag_gram, the per-column loop of the new kind
  lag_imaging_c128 / _c64          k_lag_imaging, the kernel it is modelled on (two fields in, nine planes)
  gn_<mode>                        k_gauss_newton_diagonal per mode, once per item on N cells (no field is read: 26 planes in)
  ph_<mode>_c128                   k_pseudo_hessian of the same mode on the nsrc columns, what the combine kernel is put beside

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

LINS = {'scaler': {}, 'operator': dict(linearisation='operator'), 'full': dict(linearisation='full'), 'rho': dict(linearisation='operator', parameter='rho')}
GN_MODES = {'velocity': 0, 'buoyancy': 1, 'gardner': 2, 'mass': 3, 'diagonal': 4}


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
    r = np.random.default_rng(3).standard_normal(sv.nD) + 1j * np.random.default_rng(4).standard_normal(sv.nD)
    calls = {'jtvec_full': lambda: prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full')}
    for name, kw in LINS.items():
        calls['gn_' + name] = lambda kw=kw: prob.illumination(u=F, kind='gaussNewton', **kw)
        calls['ph_' + name] = lambda kw=kw: prob.illumination(u=F, **kw)
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
    for name in LINS:
        out['gn_%s_over_jtvec' % name] = out['gn_' + name]['median_s'] / out['jtvec_full']['median_s']
        out['gn_%s_over_ph' % name] = out['gn_' + name]['median_s'] / out['ph_' + name]['median_s']
    out['all_non_negative'] = {name: bool(np.all(h >= 0)) for name, h in res.items() if name != 'jtvec_full'}
    return out


def kernels(n, nsrc, reps):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    from zephyr_amd import frechet
    lib = _lib.load()
    P = ctypes.c_void_p
    rng = np.random.default_rng(5)
    model = lambda m: dict(nz=m, nx=m, dx=10., dz=10., nPML=min(10, m - 1), freq=6., c=rng.uniform(2000., 2600., (m, m)), rho=rng.uniform(1800., 2300., (m, m)), device=0)
    sc = model(n)
    op, tiny = za.MiniZephyr(sc), za.MiniZephyr(model(3))
    h, ht = op.handle, tiny.handle
    dev = torch.device('cuda', 0)
    N = n * n
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    R = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    X = torch.empty(nsrc, dtype=torch.int32, device=dev)
    W = torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    H = torch.zeros(N, dtype=torch.float64, device=dev)
    CH = torch.from_numpy(frechet.gardnerChain(sc['c'])).to(dev)
    CU, CG = (torch.zeros(13 * N, dtype=torch.complex128, device=dev) for _ in range(2))
    C9 = torch.zeros(9 * N, dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(X.data_ptr())), h)
    u, r, p64, x, w, hh, ch, cu, cg, c9 = (P(t.data_ptr()) for t in (U, R, P64, X, W, H, CH, CU, CG, C9))
    ck = lambda rc, hd=h: _lib.check(rc, hd)
    ck(lib.helm_lag_gram_accumulate_device(h, u, min(nsrc, 4), N, cg))          # (planes of real columns for the combine kernel)

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
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        empty_call=(lambda: ck(lib.helm_lag_gram_accumulate_device(ht, u, 1, 9, cu), ht), None),
        lag_gram_c128=(lambda: ck(lib.helm_lag_gram_accumulate_device(h, u, nsrc, N, cu)), 16 * nsrc * N + 2 * 13 * 16 * N),
        lag_gram_c64=(lambda: ck(lib.helm_lag_gram_accumulate_c64_device(h, p64, x, nsrc, N, cu)), 8 * nsrc * N + 2 * 13 * 16 * N),
        lag_imaging_c128=(lambda: ck(lib.helm_lag_imaging_accumulate_device(h, u, N, r, N, nsrc, c9)), 32 * nsrc * N + 288 * N),
        lag_imaging_c64=(lambda: ck(lib.helm_lag_imaging_accumulate_c64_device(h, p64, x, N, r, N, nsrc, c9)), 24 * nsrc * N + 288 * N))
    for mode, im in GN_MODES.items():
        chm = ch if mode == 'gardner' else None
        calls['gn_' + mode] = (lambda im=im, chm=chm: ck(lib.helm_gauss_newton_diagonal_device(h, im, chm, w, cu, cg, 0.5, hh)), (26 * 16 + 24) * N)
        if im < 3:
            calls['ph_%s_c128' % mode] = (lambda im=im, chm=chm: ck(lib.helm_pseudo_hessian_accumulate_device(h, u, nsrc, N, im, chm, 0.5, w, hh)), 16 * nsrc * N + 24 * N)
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        st = stat(timed(fn))
        st['bytes'] = nbytes
        if nbytes:
            st['TBps'] = nbytes / st['median_s'] / 1e12
        res[name] = st
    for fmt in ('c128', 'c64'):
        res['lag_gram_%s_rate_over_copy' % fmt] = res['lag_gram_' + fmt]['TBps'] / res['copy_c128']['TBps']
        res['lag_gram_over_lag_imaging_' + fmt] = res['lag_gram_' + fmt]['median_s'] / res['lag_imaging_' + fmt]['median_s']
    for mode in ('velocity', 'buoyancy', 'gardner'):
        res['gn_over_ph_' + mode] = res['gn_' + mode]['median_s'] / res['ph_%s_c128' % mode]['median_s']
    del op.factors, tiny.factors
    del U, R, P64, CU, CG, C9
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--large', type=int, default=1024, help='side of the second kernel-only case (with 256 columns); 0: skip it')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gaussnewton_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['kernels'] = kernels(args.n, args.nsrc, args.kernel_reps)
    print(json.dumps({'kernels': res['kernels']}, default=float), flush=True)
    if args.large:
        res['kernels_large'] = kernels(args.large, 256, args.kernel_reps)
        print(json.dumps({'kernels_large': res['kernels_large']}, default=float), flush=True)
    cfg = job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec)
    res['routes'] = {dt: routes(cfg, args.reps, dt) for dt in ('complex128', 'complex64')}
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
