#!/usr/bin/env python3
"""dpred and mux Jtvec of a receiver array that moves with the source (geom mode 'relative') with the wavefields kept in HBM against the host path, at
config 4's survey: bench.py's 512^2 Marmousi-like model (dx = 10 m), Eurus, 8 frequencies 3 .. 10 Hz, 64 SparseKaiserSource sources and 128 receivers at
z = 20 m.  Prints one JSON object and writes it to --out (default profiles/moving_bench.json).

  relative: the receivers are a streamer behind each source, 100 m .. 1687.5 m at 12.5 m spacing; the sources run from x = 1900 m to 4920 m, so every
            receiver of every source lies inside the grid.
  fixed:    config 4's own geometry (sources 200 .. 4920 m, one line of receivers 100 .. 5020 m).
  device / host: a Helm2DProblem paired with a Helm2DSurvey, without and with hostGradient=True ('host': every frequency's N x nsrc wavefields come back
            over PCIe and scipy samples them; Jtvec images in numpy -- for a relative survey the code path of dpred before the device path took it).  Both
            in the same process, alternating, after a warm-up of each; factors rebuilt per call.  Per call and path: the median, every time, and the
            run-to-run spread (max - min) / median; their ratio host / device.

The tool runs unchanged on a checkout that predates the relative device path (there `dpred` of the relative leg is the host path on both sides): the fixed
leg of such a run is the figure the sampling kernel's extra argument is held against.
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

MODES = (('device', False), ('host', True))          # (name, hostGradient)


def job_config(n, dx, nsrc, nfreq, nrec, leg):
    import zephyr_amd as za
    from bench import build_config
    cfg = build_config(n, dx)
    width = dx * n
    if leg == 'relative':
        reach = 100.0 + 12.5 * (nrec - 1)                                     # the far end of the streamer
        assert reach + 100.0 < width - 200.0
        src = np.stack([np.linspace(reach + 212.5, width - 200.0, nsrc), np.full(nsrc, 20.0)], axis=1)
        rec = np.stack([-(100.0 + 12.5 * np.arange(nrec)), np.zeros(nrec)], axis=1)
        where = rec[None, :, :] + src[:, None, :]
        assert where[..., 0].min() >= 100.0 and where[..., 0].max() <= width - 100.0          # inside the grid for every source
    else:
        src = np.stack([np.linspace(200.0, width - 200.0, nsrc), np.full(nsrc, 20.0)], axis=1)
        rec = np.stack([np.linspace(100.0, width - 100.0, nrec), np.full(nrec, 20.0)], axis=1)
    cfg.update(Disc=za.Eurus, freqs=list(np.linspace(3.0, 10.0, nfreq)), geom=dict(src=src, rec=rec, mode=leg), batch=nsrc)
    return cfg


def summary(times):
    out = {}
    for name, _ in MODES:
        ts = times[name]
        out[name + '_s'] = float(np.median(ts))
        out[name + '_all'] = [float(t) for t in ts]
        out[name + '_spread'] = float((max(ts) - min(ts)) / np.median(ts))
    out['host_over_device'] = out['host_s'] / out['device_s']
    return out


def leg(cfg, reps):
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    pairs = {}
    for name, host in MODES:
        sc = dict(cfg, hostGradient=host)
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        assert prob._deviceGradientAvailable() is (not host)
        pairs[name] = (prob, sv)
    data, grads, resid = {}, {}, None
    for name, _ in MODES:                                      # (warm: plans, pools, first launches, the survey's cached matrices)
        prob, sv = pairs[name]
        data[name] = sv.dpred()
        if resid is None:
            rng = np.random.default_rng(4)
            resid = (rng.standard_normal(data[name].shape) + 1j * rng.standard_normal(data[name].shape)) * np.abs(data[name]).mean()
        grads[name] = prob.Jtvec(v=resid)
        del prob.factors
    td, tj = {name: [] for name, _ in MODES}, {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, _host in MODES:
            prob, sv = pairs[name]
            t0 = time.perf_counter(); sv.dpred(); td[name].append(time.perf_counter() - t0)
            del prob.factors
            t0 = time.perf_counter(); prob.Jtvec(v=resid); tj[name].append(time.perf_counter() - t0)
            del prob.factors
    nrm = np.linalg.norm
    return dict(dpred=summary(td), jtvec=summary(tj),
                dpred_device_vs_host=float(nrm(data['device'] - data['host']) / nrm(data['host'])),
                jtvec_device_vs_host=float(nrm(grads['device'] - grads['host']) / nrm(grads['host'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dx', type=float, default=10.)
    ap.add_argument('--nsrc', type=int, default=64)
    ap.add_argument('--nrec', type=int, default=128)
    ap.add_argument('--nfreq', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--legs', default='relative,fixed')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moving_bench.json'))
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    res = dict(n=args.n, dx=args.dx, nsrc=args.nsrc, nrec=args.nrec, nfreq=args.nfreq, reps=args.reps)
    for name in args.legs.split(','):
        res[name] = leg(job_config(args.n, args.dx, args.nsrc, args.nfreq, args.nrec, name), args.reps)
        print(json.dumps({name: res[name]}, default=float), flush=True)
    line = json.dumps(res, default=float)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
