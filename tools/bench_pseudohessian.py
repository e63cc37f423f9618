#!/usr/bin/env python3
"""What the pseudo-Hessian diagonal of the exact derivatives costs with the forward fields in HBM, at config 4's survey: bench.py's 512^2 Marmousi-like model
(dx = 10 m), 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU, MiniZephyr.  Prints one JSON object and writes it to --out (default
profiles/pseudohessian_bench.json).

Routes.  Two problems live side by side in one process, one with an explicit density (Gardner's formula evaluated once) and one without `rho`, each with its
store F = fieldsDevice().  Per store format, after a warm-up of each, illumination(u=F) alternates call by call between 'scaler', 'operator' (the closed form:
the energy kernel), 'full' with the explicit density, 'full' with the Gardner density and parameter='rho'.  The yardstick is the 'scaler' figure of the same run.

Kernels, on an assembled n^2 handle and nsrc random columns (wall time around the call, launch and stream synchronisation included; `empty_call` is that
overhead alone, the same entry point on a 3 x 3 handle):

  copy_c128                       a device-to-device copy of the complex128 columns, the rate everything is compared with
  energy_c128 / energy_c64        k_energy, what 'scaler' and 'operator' launch
  ph_<mode>_<fmt>_registers       k_pseudo_hessian with the coefficients built in the kernel, per mode (velocity, buoyancy, gardner) and store format
  ph_<mode>_<fmt>_packed          the same reading the coefficients from the array of helm_pseudo_hessian_coefficients_device (coefficients_<mode>: that
                                  kernel alone, once per operator and mode)
  nine_colour_<mode>              the composition from the kernels that were there: per colour indicator k_velocity_planes / k_buoyancy_planes,
                                  k_stencil_sources into a scratch of nsrc columns, and -- as nothing on the device squares and box-sums that scratch --
                                  k_energy over it standing for the read-back; nine passes that each read U, write R and read R.  It is a cost model of the
                                  composition, not a result: the box sum and the scatter by colour are left out, in its favour.

Per figure: the median, every time, the run-to-run spread (max - min) / median, the bytes the fused kernel has to move (the fields once) and the rate.
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

VARIANTS = {'scaler': ('rho', {}), 'operator': ('rho', dict(linearisation='operator')), 'full': ('rho', dict(linearisation='full')),
            'full_gardner': ('gardner', dict(linearisation='full')), 'rho': ('rho', dict(linearisation='operator', parameter='rho'))}
MODES = {'velocity': 0, 'buoyancy': 1, 'gardner': 2}


def routes(cfg, reps, dtype):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    c = np.asarray(cfg['c'])
    pairs = {}
    for name, extra in (('rho', dict(rho=310. * np.real(c) ** 0.25)), ('gardner', {})):
        sc = dict(cfg, Disc=za.MiniZephyr, fieldsDtype=dtype)
        sc.pop('rho', None)
        sc.update(extra)
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        pairs[name] = (prob, prob.fieldsDevice())
    times, res = {}, {}

    def one_round():
        for var, (which, kw) in VARIANTS.items():
            prob, F = pairs[which]
            t0 = time.perf_counter()
            res[var] = prob.illumination(u=F, **kw)
            times.setdefault(var, []).append(time.perf_counter() - t0)
    one_round()
    times.clear()
    for _ in range(reps):
        one_round()
    for prob, F in pairs.values():
        F.release()
        del prob.factors
    out = {name: stat(ts) for name, ts in times.items()}
    for var in VARIANTS:
        if var != 'scaler':
            out[var + '_over_scaler'] = out[var]['median_s'] / out['scaler']['median_s']
    out['all_positive'] = {var: bool(np.all(h > 0)) for var, h in res.items()}
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
    E = torch.empty(33 * N, dtype=torch.complex128, device=dev)
    C9 = torch.empty(9 * N, dtype=torch.complex128, device=dev)
    iz, ix = np.divmod(np.arange(N), n)
    colours = [torch.from_numpy(((iz % 3 == a) & (ix % 3 == b)).astype(np.float64)).to(dev) for a in range(3) for b in range(3)]
    chained = [CH * v for v in colours]
    torch.cuda.synchronize(dev)
    _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(X.data_ptr())), h)
    u, r, p64, x, w, hh, ch, e, c9 = (P(t.data_ptr()) for t in (U, R, P64, X, W, H, CH, E, C9))
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

    def nine_colour(mode):
        def run():
            for v, cv in zip(colours, chained):
                if mode == 'buoyancy':
                    ck(lib.helm_buoyancy_planes_device(h, P(v.data_ptr()), c9))
                else:
                    ck(lib.helm_velocity_planes_device(h, P(v.data_ptr()), P(cv.data_ptr()) if mode == 'gardner' else None, c9))
                ck(lib.helm_stencil_sources_device(h, u, nsrc, N, c9, 1.0, 0.0, 0, r, N))
                ck(lib.helm_energy_accumulate_device(h, r, nsrc, N, 0.5, w, hh))
        return run
    fields = {'c128': 16 * nsrc * N + 24 * N, 'c64': 8 * nsrc * N + 24 * N}
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        energy_c128=(lambda: ck(lib.helm_energy_accumulate_device(h, u, nsrc, N, 0.5, w, hh)), fields['c128']),
        energy_c64=(lambda: ck(lib.helm_energy_accumulate_c64_device(h, p64, x, nsrc, N, 0.5, w, hh)), fields['c64']),
        empty_call=(lambda: ck(lib.helm_pseudo_hessian_accumulate_device(ht, u, 1, 9, 0, None, 0.5, None, hh), ht), None))
    for mode, im in MODES.items():
        chm = ch if mode == 'gardner' else None
        ncoef = 10 if mode == 'velocity' else 33
        calls['coefficients_' + mode] = (lambda im=im, chm=chm: ck(lib.helm_pseudo_hessian_coefficients_device(h, im, chm, e)), 16 * ncoef * N)
        calls['ph_%s_c128_registers' % mode] = (lambda im=im, chm=chm: ck(lib.helm_pseudo_hessian_accumulate_device(h, u, nsrc, N, im, chm, 0.5, w, hh)), fields['c128'])
        calls['ph_%s_c64_registers' % mode] = (lambda im=im, chm=chm: ck(lib.helm_pseudo_hessian_accumulate_c64_device(h, p64, x, nsrc, N, im, chm, 0.5, w, hh)),
                                               fields['c64'])
        # (timed after coefficients_<mode>, which leaves the array of this mode in E)
        calls['ph_%s_c128_packed' % mode] = (lambda im=im: ck(lib.helm_pseudo_hessian_accumulate_packed_device(h, u, nsrc, N, im, None, e, 0.5, w, hh)),
                                             fields['c128'] + 16 * ncoef * N)
        calls['ph_%s_c64_packed' % mode] = (lambda im=im: ck(lib.helm_pseudo_hessian_accumulate_packed_c64_device(h, p64, x, nsrc, N, im, None, e, 0.5, w, hh)),
                                            fields['c64'] + 16 * ncoef * N)
        calls['nine_colour_' + mode] = (nine_colour(mode), 9 * (48 * nsrc * N + 176 * N))
    res = dict(n=n, nsrc=nsrc, reps=reps)
    for name, (fn, nbytes) in calls.items():
        st = stat(timed(fn))
        st['bytes'] = nbytes
        if nbytes:
            st['TBps'] = nbytes / st['median_s'] / 1e12
        res[name] = st
    for mode in MODES:
        for fmt in ('c128', 'c64'):
            for place in ('registers', 'packed'):
                k = 'ph_%s_%s_%s' % (mode, fmt, place)
                res[k]['rate_over_copy'] = res[k]['TBps'] / res['copy_c128']['TBps']
                res[k]['over_energy'] = res[k]['median_s'] / res['energy_' + fmt]['median_s']
        res['nine_colour_%s_over_fused' % mode] = res['nine_colour_' + mode]['median_s'] / res['ph_%s_c128_registers' % mode]['median_s']
        res['packed_over_registers_%s' % mode] = res['ph_%s_c128_packed' % mode]['median_s'] / res['ph_%s_c128_registers' % mode]['median_s']
    del op.factors, tiny.factors
    del U, R, P64, E, C9
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pseudohessian_bench.json'))
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
