#!/usr/bin/env python3
"""Write tests/golden/g13_operator_device.npz: what the device routes of JvecBorn / Jtvec(adjoint='transpose') / Hvec give with linearisation='scaler' and
'operator' (and 'operator' with parameter='rho') on the 37 x 53 survey of tests/frechet_cases.py, complex128 store, one GPU  --  test infrastructure.

The recording is made on the commit BEFORE linearisation='full' is added; tests/test_gpu_full.py asserts that the same calls still give the same bits.  It is
this project's own output (tests/full_cases.recorded_products states the inputs); run it again only when a change is MEANT to alter those routes.

    python tools/record_operator_device.py [file]     (on a machine with an MI355X, after __graft_entry__.build(); default: the golden file itself)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['HELM_DEVICES'] = '0'

import numpy as np                                      # noqa: E402
from tests import full_cases as xc                      # noqa: E402


def main():
    out = {}
    for mode in xc.RECORDED_MODES:
        for key, val in xc.recorded_products(mode).items():
            out['%s/%s' % (mode, key)] = val
    path = sys.argv[1] if len(sys.argv) > 1 else xc.RECORDING
    np.savez(path, **out)
    print('%s: %d arrays, %d bytes' % (os.path.relpath(path, ROOT), len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
