"""CPU: the host side of the device-resident 2.5-D ky sum -- the two new C-ABI entry points refuse bad arguments before they touch a device, the order
of prefactor / solve steps of the ky loop, and the composite's choice between the device sum and the reference's host reduction."""
import ctypes
import os

import numpy as np
import pytest

import zephyr_amd as za
from zephyr_amd import _lib
from zephyr_amd.minizephyr import ky_schedule, KY_GROUP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_new_entry_points_refuse_bad_arguments_without_a_gpu(helm_lib):
    assert 'helm_axpby_device' in _lib.exported_symbols() and 'helm_sample_accumulate_device' in _lib.exported_symbols()
    p = ctypes.c_void_p
    fake_op, a, b = p(0x1000), p(0x2000), p(0x3000)          # never dereferenced: every call below must return before it looks at the handle
    ax = helm_lib.helm_axpby_device
    assert ax(None, 1., 0., a, 0., 0., b, 16) == -1
    assert ax(fake_op, 1., 0., None, 0., 0., b, 16) == -1
    assert ax(fake_op, 1., 0., a, 0., 0., None, 16) == -1
    assert ax(fake_op, 1., 0., a, 0., 0., b, 0) == -1
    assert ax(fake_op, 1., 0., a, 0., 0., b, -5) == -1
    assert ax(fake_op, 1., 0., a, 1., 0., a, 16) == -1       # X == Y
    assert ax(fake_op, 1., 0., p(0x2008), 1., 0., b, 16) == -1      # not on a 16-byte boundary
    sa = helm_lib.helm_sample_accumulate_device
    good = dict(op=fake_op, dU=a, nsrc=2, ld=8, rowptr=a, col=a, val=a, nrec=3, out=b)

    def call(**kw):
        v = dict(good, **kw)
        return sa(v['op'], v['dU'], v['nsrc'], v['ld'], v['rowptr'], v['col'], v['val'], v['nrec'], 1., 0., 0., 0., v['out'])
    for key in ('op', 'dU', 'rowptr', 'col', 'val', 'out'):
        assert call(**{key: None}) == -1, key
    assert call(nsrc=0) == -1 and call(nrec=0) == -1 and call(nsrc=-1) == -1 and call(nrec=-2) == -1


@pytest.mark.parametrize('group', [1, 2, 4])
def test_ky_schedule_prefactors_every_ky_once_before_its_solve(group):
    for nky in range(1, 22):
        steps = ky_schedule(nky, group)
        prefactored, solved, pending_max = [], [], 0
        for step, arg in steps:
            if step == 'prefactor':
                assert 1 <= len(arg) <= group
                prefactored.extend(arg)
            else:
                assert step == 'solve'
                assert arg in prefactored, 'ky %d solved before it was prefactored' % arg
                solved.append(arg)
            pending_max = max(pending_max, len(prefactored) - len(solved))
        assert sorted(prefactored) == list(range(nky)) and len(set(prefactored)) == nky          # exactly once
        assert solved == list(range(nky))                                                          # the order of the reference's sum
        assert pending_max <= 2 * group
        first_solve = [s for s, _ in steps].index('solve')          # there IS look-ahead: the second group is on its way before the first solve
        assert sum(len(a) for _, a in steps[:first_solve]) == min(nky, 2 * group)
    assert KY_GROUP in (1, 2, 4) and ky_schedule(5) == ky_schedule(5, KY_GROUP)


def test_composite_interface_and_host_branch_of_the_cpu_double():
    from tests.doubles import OracleMiniZephyr25D
    for name in ('solveDevice', 'sampleSumDevice', 'prefactor', 'reserve', 'rhsFromSparseDevice', 'rhsSupportFromSparse', 'imagingAccumulateDevice'):
        assert name in za.MiniZephyr25D.__dict__, name            # the composite's own, not what BaseDiscretization would lend it
    g = np.load(os.path.join(GOLD, 'g11_25d_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freq=float(g['freqs'][0]), nky=3)
    real = za.MiniZephyr25D(sc)
    assert real.deviceCapable and real.kyOnDevice and real.kySumOnDevice and not real.kyRelease
    assert not za.MiniZephyr25D(dict(sc, kyOnDevice=False)).kySumOnDevice
    assert za.MiniZephyr25D(dict(sc, kyRelease=True)).kyRelease
    assert 'kyOnDevice' not in za.MiniZephyr25D(dict(sc, kyOnDevice=False)).systemConfig             # the ky sub-problems do not see the composite's own keys
    op = OracleMiniZephyr25D(sc)
    assert not op.deviceCapable and not op.kySumOnDevice and not op._onDevice()
    assert not op.factors
    q = za.SimpleSource(sc)(np.array([[200., 150.], [330., 240.]]))
    u = op * q
    ref = None
    for sub in op.subProblems:
        t = sub * q
        ref = t if ref is None else np.add(ref, t)
    ref = op.scaleTerm * ref
    assert u.shape == (nz * nx, 2) and np.array_equal(u, ref)                      # the old branch, bit for bit
    q1 = np.asarray(q.todense() if hasattr(q, 'todense') else q)[:, 0]
    u1 = op * q1
    assert u1.shape == (nz * nx,) and np.linalg.norm(u1 - ref[:, 0]) <= 1e-10 * np.linalg.norm(ref[:, 0])
