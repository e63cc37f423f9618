#!/usr/bin/env python3
"""What keeping the forward wavefields in HBM buys a misfit-and-gradient evaluation, at config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m),
Eurus, 8 frequencies 3 .. 10 Hz, 64 sources, a fixed line of 128 receivers, one GPU.  Prints one JSON object and writes it to --out (default
profiles/fields_bench.json).

Three sequences, each one model evaluation with fresh factors (del prob.factors before it, none inside it), alternating run by run in one process after a
warm-up of each:

  mux:        dpred()  then  Jtvec(None, r)                               -- 3 nsrc columns solved per frequency
  fields128:  F = fieldsDevice(); dpred(u=F); Jtvec(None, r, u=F)         -- 2 nsrc columns, the store complex128
  fields64:   the same with fieldsDtype='complex64'                        -- the store half the size, one pack per item

Per sequence and part: the median, every time, and the run-to-run spread (max - min) / median.  Then the three kernels of the complex64 store alone on the
buffers of one frequency (nsrc columns of n^2 points): wall time around the call (each returns when its result is complete, so launch and stream
synchronisation are included), the bytes each has to move, and the rate against a device-to-device copy of the same wavefield buffer measured the same way.
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

SEQS = ('mux', 'fields128', 'fields64')


def job_config(n, dx, nsrc, nfreq, nrec):
    import zephyr_amd as za
    from bench import build_config
    cfg = build_config(n, dx)
    width = dx * n
    src = np.stack([np.linspace(200.0, width - 200.0, nsrc), np.full(nsrc, 20.0)], axis=1)
    rec = np.stack([np.linspace(100.0, width - 100.0, nrec), np.full(nrec, 20.0)], axis=1)
    cfg.update(Disc=za.Eurus, freqs=list(np.linspace(3.0, 10.0, nfreq)), geom=dict(src=src, rec=rec, mode='fixed'), batch=nsrc)
    return cfg


def stat(ts):
    return dict(median_s=float(np.median(ts)), all_s=[float(t) for t in ts], spread=float((max(ts) - min(ts)) / np.median(ts)))


def run_sequence(name, prob, sv, resid):
    'one model evaluation; returns (times of its parts, data, gradient)'
    del prob.factors
    t = {}
    t0 = time.perf_counter()
    if name == 'mux':
        d = sv.dpred()
        t['dpred'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        g = prob.Jtvec(None, resid) if resid is not None else None
        t['jtvec'] = time.perf_counter() - t1
    else:
        F = prob.fieldsDevice()
        t['fields'] = time.perf_counter() - t0
        t1 = time.perf_counter()
        d = sv.dpred(u=F)
        t['dpred'] = time.perf_counter() - t1
        t1 = time.perf_counter()
        g = prob.Jtvec(None, resid, u=F) if resid is not None else None
        t['jtvec'] = time.perf_counter() - t1
        F.release()
    t['total'] = time.perf_counter() - t0
    return t, d, g


def sequences(cfg, reps):
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    pairs = {}
    for name in SEQS:
        sc = dict(cfg, fieldsDtype='complex64' if name == 'fields64' else 'complex128')
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable()
        pairs[name] = (prob, sv)
    _, d0, _ = run_sequence('mux', *pairs['mux'], None)
    rng = np.random.default_rng(4)
    resid = (rng.standard_normal(d0.shape) + 1j * rng.standard_normal(d0.shape)) * np.abs(d0).mean()
    out = {}
    for name in SEQS:                                         # (warm: plans, pools, first launches, the survey's cached matrices)
        _, d, g = run_sequence(name, *pairs[name], resid)
        out[name] = (d, g)
    times = {name: {} for name in SEQS}
    for _ in range(reps):
        for name in SEQS:
            t, _, _ = run_sequence(name, *pairs[name], resid)
            for part, v in t.items():
                times[name].setdefault(part, []).append(v)
    for name in SEQS:
        del pairs[name][0].factors
    nrm = np.linalg.norm
    res = {name: {part: stat(ts) for part, ts in times[name].items()} for name in SEQS}
    gmux = out['mux'][1].real                                 # (the mux branch returns the complex sum, the u-given branch its real part: problem.py:162)
    res['agreement'] = dict(
        dpred_fields128_vs_mux=float(nrm(out['fields128'][0] - out['mux'][0]) / nrm(out['mux'][0])),
        dpred_fields64_vs_mux=float(nrm(out['fields64'][0] - out['mux'][0]) / nrm(out['mux'][0])),
        jtvec_fields128_vs_mux_real=float(nrm(out['fields128'][1] - gmux) / nrm(gmux)),
        jtvec_fields64_vs_fields128=float(nrm(out['fields64'][1] - out['fields128'][1]) / nrm(out['fields128'][1])))
    for name in ('fields128', 'fields64'):
        res[name]['total_over_mux'] = res[name]['total']['median_s'] / res['mux']['total']['median_s']
    return res


def kernels(n, nsrc, nrec, reps):
    'the three kernels of the complex64 store on one frequency\'s buffers, against a device-to-device copy of the complex128 wavefields'
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    op = za.MiniZephyr(dict(nx=n, nz=n, dx=10., dz=10., c=2500., freq=5., nPML=10))
    dev = torch.device('cuda', op.device)
    N = int(op.nrow)
    h = op.handle
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    UB = torch.view_as_complex(torch.randn((nsrc, N, 2), dtype=torch.float64, device=dev, generator=gen))
    U2 = torch.empty_like(U)
    P64 = torch.empty((nsrc, N), dtype=torch.complex64, device=dev)
    E = torch.empty(nsrc, dtype=torch.int32, device=dev)
    scaler = torch.view_as_complex(torch.randn((N, 2), dtype=torch.float64, device=dev, generator=gen))
    G = torch.zeros(N, dtype=torch.complex128, device=dev)
    # a receiver line like the survey's: nrec rows of 81 entries
    rng = np.random.default_rng(2)
    nnz = 81
    rowptr = torch.arange(0, (nrec + 1) * nnz, nnz, dtype=torch.int64, device=dev)
    col = torch.from_numpy(rng.integers(0, N, nrec * nnz).astype(np.int64)).to(dev)
    val = torch.view_as_complex(torch.randn((nrec * nnz, 2), dtype=torch.float64, device=dev, generator=gen))
    out = torch.empty((nrec, nsrc), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)

    def timed(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return ts

    def copy():
        U2.copy_(U)
        torch.cuda.synchronize(dev)
    calls = dict(
        copy_c128=(copy, 32 * nsrc * N),
        pack_c64=(lambda: _lib.check(lib.helm_pack_c64_device(h, P(U.data_ptr()), nsrc, N, P(P64.data_ptr()), P(E.data_ptr())), h), (16 + 16 + 8) * nsrc * N),
        imaging_c64=(lambda: _lib.check(lib.helm_imaging_accumulate_c64_device(h, P(P64.data_ptr()), P(E.data_ptr()), P(UB.data_ptr()), nsrc, P(scaler.data_ptr()),
                                                                           P(G.data_ptr())), h), (8 + 16) * nsrc * N + 48 * N),
        imaging_c128=(lambda: op.imagingAccumulateDevice(U.data_ptr(), UB.data_ptr(), nsrc, scaler.data_ptr(), G.data_ptr()), 32 * nsrc * N + 48 * N),
        sample_rows_c64=(lambda: _lib.check(lib.helm_sample_rows_c64_device(h, P(P64.data_ptr()), P(E.data_ptr()), nsrc, N, P(rowptr.data_ptr()), P(col.data_ptr()),
                                                                            P(val.data_ptr()), nrec, 0, 1.0, 0.0, 0.0, 0.0, P(out.data_ptr())), h), None),
        sample_rows_c128=(lambda: _lib.check(lib.helm_sample_rows_device(h, P(U.data_ptr()), nsrc, N, P(rowptr.data_ptr()), P(col.data_ptr()), P(val.data_ptr()), nrec,
                                                                         0, 1.0, 0.0, 0.0, 0.0, P(out.data_ptr())), h), None))
    res = dict(n=n, nsrc=nsrc, nrec=nrec, entries_per_row=nnz, reps=reps)
    for name, (fn, nbytes) in calls.items():
        ts = timed(fn)
        r = stat(ts)
        r['bytes'] = nbytes
        if nbytes:
            r['TBps'] = nbytes / r['median_s'] / 1e12
        res[name] = r
    for name in ('pack_c64', 'imaging_c64', 'imaging_c128'):
        res[name]['rate_over_copy'] = res[name]['TBps'] / res['copy_c128']['TBps']
    del op.factors
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fields_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    res['sequences'] = sequences(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec), args.reps)
    print(json.dumps({'sequences': res['sequences']}, default=float), flush=True)
    res['kernels'] = kernels(args.n, args.nsrc, args.nrec, args.kernel_reps)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
