#!/usr/bin/env python3
"""2.5-D (MiniZephyr25D) with the ky sum kept in HBM against the host reduction, at config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m),
8 frequencies 3 .. 10 Hz, 64 SparseKaiserSource sources and 128 receivers at z = 20 m, nky = 8.  Prints one JSON object and writes it to --out.

  mul:     wall time of `MultiFreq(Disc=MiniZephyr25D) * q`, results drained to the host as a caller gets them.
  dpred / jtvec: a Helm25DProblem paired with a Helm25DSurvey (model set once, factors rebuilt per call).
           Each of the three with kyOnDevice True ('device') and False ('host': every ky returns its wavefields over PCIe, numpy adds them -- the code path
           before the device sum existed) in the same process, alternating, after a warm-up of each; their ratio host / device is reported.
  axpby:   helm_axpby_device alone (beta != 0: 48 B per element) on 64 x 512^2 and 512 x 1024^2 elements: wall time around the call, which returns
           when the pass is done; GB/s and the fraction of the measured float4-copy rate (6.29 TB/s) and of the 8 TB/s peak.

For kernel times, run `--only axpby` (and `--only problem`) under `rocprofv3 --kernel-trace --stats` in a separate run.
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

PEAK_BW, COPY_BW = 8e12, 6.29e12
MODES = (('device', True), ('host', False))


def job_config(n, dx, nsrc, nfreq, nky, release):
    from bench import build_config
    from zephyr_amd import MiniZephyr25D
    cfg = build_config(n, dx)
    src = np.stack([np.linspace(200.0, dx * n - 200.0, nsrc), np.full(nsrc, 20.0)], axis=1)
    rec = np.stack([np.linspace(100.0, dx * n - 100.0, 128), np.full(128, 20.0)], axis=1)
    cfg.update(Disc=MiniZephyr25D, nky=nky, freqs=list(np.linspace(3.0, 10.0, nfreq)), geom=dict(src=src, rec=rec, mode='fixed'), kyRelease=bool(release))
    return cfg


def summary(times):
    out = {}
    for name, _ in MODES:
        out[name + '_s'] = float(np.median(times[name]))
        out[name + '_all'] = [float(t) for t in times[name]]
    out['host_over_device'] = out['host_s'] / out['device_s']
    return out


def mul_leg(cfg, reps):
    from zephyr_amd import MultiFreq
    from zephyr_amd.survey import Helm25DSurvey
    q = Helm25DSurvey(cfg).getSources()
    wrappers = {name: MultiFreq(dict(cfg, kyOnDevice=on)) for name, on in MODES}

    def run(sysw):
        t0 = time.perf_counter()
        for u in sysw * q:
            del u
        t = time.perf_counter() - t0
        del sysw.factors
        return t
    for name, _ in MODES:
        run(wrappers[name])                                    # (warm: plans, pools, first launches)
    times = {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, _on in MODES:
            times[name].append(run(wrappers[name]))
    return summary(times)


def problem_leg(cfg, reps):
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    pairs = {}
    for name, on in MODES:
        sc = dict(cfg, kyOnDevice=on)
        prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable() is on
        pairs[name] = (prob, sv)
    data, grads, resid = {}, {}, None
    for name, _ in MODES:                                      # (warm)
        prob, sv = pairs[name]
        data[name] = sv.dpred()
        resid = np.ones(data[name].shape, dtype=np.complex128)
        grads[name] = prob.Jtvec(v=resid)
        del prob.factors
    td, tj = {name: [] for name, _ in MODES}, {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, _on in MODES:
            prob, sv = pairs[name]
            t0 = time.perf_counter(); sv.dpred(); td[name].append(time.perf_counter() - t0)
            del prob.factors
            t0 = time.perf_counter(); prob.Jtvec(v=resid); tj[name].append(time.perf_counter() - t0)
            del prob.factors
    nrm = np.linalg.norm
    return dict(dpred=summary(td), jtvec=summary(tj),
                dpred_device_vs_host=float(nrm(data['device'] - data['host']) / nrm(data['host'])),
                jtvec_device_vs_host=float(nrm(grads['device'] - grads['host']) / nrm(grads['host'])))


def axpby_leg(reps, sizes):
    import torch
    from zephyr_amd import MiniZephyr, _lib
    lib = _lib.load()
    op = MiniZephyr(dict(nx=32, nz=32, dx=10., dz=10., c=2500., freq=5., nPML=4))
    dev = torch.device('cuda', op.device)
    st = np.exp(1j * np.pi) / (4 * np.pi)
    out = []
    for label, n in sizes:
        X = torch.empty(n, dtype=torch.complex128, device=dev).fill_(1.0 + 0.5j)
        Y = torch.empty(n, dtype=torch.complex128, device=dev).fill_(0.25 - 1.0j)
        torch.cuda.synchronize(dev)

        def call():
            _lib.check(lib.helm_axpby_device(op.handle, st.real, st.imag, ctypes.c_void_p(X.data_ptr()), 1.0, 0.0, ctypes.c_void_p(Y.data_ptr()), n), op.handle)
        call()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        byts = 48 * n
        out.append(dict(label=label, n=n, bytes=byts, wall_ms=1e3 * t, wall_ms_all=[1e3 * x for x in ts], GBps=byts / t / 1e9,
                        fraction_of_copy_rate=byts / t / COPY_BW, fraction_of_peak=byts / t / PEAK_BW))
        del X, Y
    del op.factors
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--nky', type=int, default=8)
    ap.add_argument('--release', action='store_true', help='kyRelease = True (a ky operator is destroyed after its last solve of a call)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', choices=['all', 'mul', 'problem', 'axpby'], default='all')
    ap.add_argument('--axpby-small', action='store_true', help='axpby leg on 64 x 512^2 elements only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nfreq=args.nfreq, nky=args.nky, kyRelease=bool(args.release), reps=args.reps)
    cfg = job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nky, args.release)
    if args.only in ('all', 'axpby'):
        sizes = [('64 x 512^2', 64 * 512 * 512)] + ([] if args.axpby_small else [('512 x 1024^2', 512 * 1024 * 1024)])
        res['axpby'] = axpby_leg(max(5, args.reps), sizes)
        print(json.dumps(dict(axpby=res['axpby']), default=float), flush=True)
    if args.only in ('all', 'mul'):
        res['mul'] = mul_leg(cfg, args.reps)
        print(json.dumps(dict(mul=res['mul']), default=float), flush=True)
    if args.only in ('all', 'problem'):
        res.update(problem_leg(cfg, args.reps))
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
