#!/usr/bin/env python3
"""Write tests/golden/g12_moving_survey.npz from the REAL reference (dev container only)  --  test infrastructure.

The g6 model with its relative geometry (a receiver array that moves with the source; every input is read from g6_survey.npz and not stored again):
a seeded residual, the reference's gradient by both branches of Jtvec (`g_mux`, `g_u`) and its `dpred`.  The reference is imported through the
stand-in packages of oracle/refshim, as oracle/make_golden.py does; nothing under oracle/ is changed.  Only data is written.

    PYTHONDONTWRITEBYTECODE=1 ZEPHYR_REFERENCE=<checkout of the reference> python tools/make_golden_moving.py

Nothing here runs on the GPU box and the product package never imports it.
"""
import os
import sys
import warnings

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('ZEPHYR_REFERENCE')
if not REF or not os.path.isdir(os.path.join(REF, 'zephyr')):
    sys.exit('set ZEPHYR_REFERENCE to a checkout of the reference (the directory that holds the `zephyr` package)')
sys.path[:0] = [os.path.join(ROOT, 'oracle', 'refshim'), REF, ROOT]
warnings.simplefilter('ignore')

import numpy as np                                      # noqa: E402
import zephyr.backend as zb                             # noqa: E402  (the reference)
from zephyr.middleware import Helm2DProblem, Helm2DSurvey          # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def main():
    g = np.load(os.path.join(GOLD, 'g6_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=zb.MiniZephyrHD, parallel=False,
              sterms=g['sterms'], geom=dict(src=g['src'], rec=g['rec_relative'], mode='relative'))
    prob, surv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(surv)
    d = surv.dpred()
    assert np.array_equal(d, g['dpred_relative'])       # the same configuration as g6's relative leg
    rng = np.random.default_rng(1207)
    resid = (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) * np.abs(d).mean()
    g_mux = prob.Jtvec(None, resid)
    uF = [np.asarray(x) for x in prob.lazyFields()]
    g_u = prob.Jtvec(None, resid, u=uF)
    out = os.path.join(GOLD, 'g12_moving_survey.npz')
    np.savez_compressed(out, resid=resid, g_mux=np.asarray(g_mux), g_u=np.asarray(g_u), dpred=d)
    print('%s: %d bytes (g6_survey.npz: %d)' % (os.path.relpath(out, ROOT), os.path.getsize(out), os.path.getsize(os.path.join(GOLD, 'g6_survey.npz'))))


if __name__ == '__main__':
    main()
