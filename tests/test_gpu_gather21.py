"""GPU: the ring x separator block F21 of a front gathered by the product G21 = F21 F11^-1 that is its only reader (k_zgemm3<.., 3, ..>, GemmRows::gather21;
HELM_ND_GATHER21) instead of being written by the build pass and read back -- against the path it replaces (the factors are meant to be the same bits) and
against the sparse LU of the oracle's matrix, on grids whose plans (checked here, on the host) hold separator fronts of 17-64 cells, fronts padded below
their group's size, fronts on the grid's edge with short rings, and both leaf and separator children; at the default routing; with dozens of fronts flagged
and re-eliminated; for several operators in the same launches; and on a transposed handle.  HELM_ND_GATHER21_SMAX=4096 with HELM_ND_FUSEDSEP=0 sends every
separator level that has a ring through the new mode, the fronts of 3-16 cells included."""
import ctypes

import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p

CASES = [('MiniZephyr', 64, 64, (0, 0, 0, 0)), ('Eurus', 70, 90, (0, 0, 0, 0)), ('MiniZephyr', 41, 150, (1, 0, 0, 1)),
         ('Eurus', 128, 128, (0, 0, 0, 0)), ('MiniZephyr', 57, 33, (0, 1, 1, 0))]


def nrm(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def gather_fronts(lib, nz, nx, leaf):
    'rows {z0, z1, x0, x1, cut, pos, s, m, kid0, kid1, smax, mmax} of the separator fronts with a ring, and the whole plan (helm_direct_plan: host only)'
    n = lib.helm_direct_plan(nz, nx, leaf, None, 0)
    plan = np.zeros((n, 12), dtype=np.int32)
    assert lib.helm_direct_plan(nz, nx, leaf, plan.ctypes.data_as(P), n) == n
    take = (plan[:, 4] >= 0) & (plan[:, 11] > 0)
    return plan[take], plan


def assert_plan_covers_the_cases(lib, nz, nx, leaf):
    fr, plan = gather_fronts(lib, nz, nx, leaf)
    assert ((fr[:, 10] > 16) & (fr[:, 10] <= 64)).any()                     # the levels the path is the default for
    assert (fr[:, 10] <= 16).any()                                          # the small separators, which take it with the fused kernel off
    assert (fr[:, 6] < fr[:, 10]).any()                                     # fronts padded below smax
    assert (fr[:, 7] < fr[:, 11]).any()                                     # short rings: fronts on the grid's edge
    assert any(plan[r[8], 4] < 0 for r in fr) and any(plan[r[8], 4] >= 0 for r in fr)      # leaf children and separator children
    return fr


def case_setup(cls, nz, nx, fs):
    'model, sources and oracle planes of tests/test_gpu_fused_sep.py'
    import zephyr_amd as za
    rng = np.random.default_rng(nz * 3 + nx)
    c = 1700. + 2500. * rng.random((nz, nx))
    rho = 1000. + 500. * rng.random((nz, nx))
    cfg = dict(nx=nx, nz=nz, dx=10., dz=12., c=c, rho=rho, freq=11., nPML=6, rtol=1e-11, method='direct', freeSurf=fs)
    q = za.SimpleSource(cfg)(np.array([[nx * 3.3, nz * 4.1], [nx * 6.0, nz * 7.7], [25., 30.]]))
    if cls == 'MiniZephyr':
        C = ho.minizephyr_coefficients(nz, nx, c, rho, 11., dx=10., dz=12., nPML=6, freeSurf=fs)
    else:
        C = ho.eurus_coefficients(nz, nx, c, rho, 11., dx=10., dz=12., nPML=6)
    return cfg, q, C


def every_level(monkeypatch):
    monkeypatch.setenv('HELM_ND_GATHER21_SMAX', '4096')
    monkeypatch.setenv('HELM_ND_FUSEDSEP', '0')


@pytest.mark.parametrize('leaf', [8, 4])
@pytest.mark.parametrize('cls,nz,nx,fs', CASES)
def test_gathered_f21_gives_the_factors_of_the_built_f21_and_matches_sparse_lu(helm_lib, monkeypatch, cls, nz, nx, fs, leaf):
    import zephyr_amd as za
    assert_plan_covers_the_cases(helm_lib, nz, nx, leaf)
    every_level(monkeypatch)
    monkeypatch.setenv('HELM_ND_LEAF', str(leaf))
    cfg, q, C = case_setup(cls, nz, nx, fs)
    monkeypatch.setenv('HELM_ND_GATHER21', '1')
    op = getattr(za, cls)(cfg)
    u = np.array(op * q)
    ref = ho.DirectOperator(C, eurus=(cls == 'Eurus')) * q
    print('%s %dx%d leaf %d: against LU %.2e, worst relres %.2e' % (cls, nz, nx, leaf, nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert nrm(u, ref) <= 1e-8
    assert all(i['status'] == 0 and i['relres'] <= 1e-11 for i in op.lastInfo), op.lastInfo
    monkeypatch.setenv('HELM_ND_GATHER21', '0')
    op2 = getattr(za, cls)(cfg)
    u2 = np.array(op2 * q)
    print('   gathered against built %.2e, bit for bit: %s' % (nrm(u, u2), np.array_equal(u, u2)))
    assert np.array_equal(u, u2)
    del op.factors, op2.factors


def test_default_routing_fused_kernel_below_gathered_f21_above(helm_lib, monkeypatch):
    'neither switch set, the fused small-separator kernel at its default: what the benchmark runs, on against off'
    import zephyr_amd as za
    for name in ('HELM_ND_GATHER21', 'HELM_ND_GATHER21_SMAX', 'HELM_ND_FUSEDSEP', 'HELM_ND_FUSEDSEP_MIN'):
        monkeypatch.delenv(name, raising=False)
    cls, nz, nx, fs = CASES[3]
    assert_plan_covers_the_cases(helm_lib, nz, nx, 8)
    cfg, q, C = case_setup(cls, nz, nx, fs)
    op = getattr(za, cls)(cfg)
    u = np.array(op * q)
    ref = ho.DirectOperator(C, eurus=True) * q
    print('default routing: against LU %.2e, worst relres %.2e' % (nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert nrm(u, ref) <= 1e-8
    assert all(i['status'] == 0 and i['relres'] <= 1e-11 for i in op.lastInfo), op.lastInfo
    monkeypatch.setenv('HELM_ND_GATHER21', '0')
    op2 = getattr(za, cls)(cfg)
    u2 = np.array(op2 * q)
    assert np.array_equal(u, u2)
    del op.factors, op2.factors


@pytest.mark.parametrize('seed', [0, 1])
def test_flagged_fronts_are_rebuilt_whole_before_their_f21_is_taken(helm_lib, monkeypatch, seed):
    """the two seeded models of test_fused_levels_with_dozens_of_fronts_flagged_and_reeliminated (seed 0: MiniZephyr with a free surface, seed 1: Eurus) with the
    threshold at 30: stabilise_group copies F21 out of the arena, where with the path on only its own rebuild of the front has written it"""
    import zephyr_amd as za
    rng = np.random.default_rng(77 + seed)
    nz, nx = int(rng.integers(150, 260)), int(rng.integers(150, 300))
    c = 1600. + 2200. * rng.random((nz, nx))
    rho = 1000. + 600. * rng.random((nz, nx))
    f = float(rng.uniform(8., 20.))
    nrhs = int(rng.integers(3, 40))
    q = np.zeros((nz * nx, nrhs), complex)
    q[rng.integers(0, nz * nx, nrhs), np.arange(nrhs)] = rng.standard_normal(nrhs) + 1j * rng.standard_normal(nrhs)
    fr, _ = gather_fronts(helm_lib, nz, nx, 8)
    assert len(fr) >= 200 and (fr[:, 10] > 64).any() and ((fr[:, 10] > 16) & (fr[:, 10] <= 64)).any()
    monkeypatch.setenv('HELM_ND_STABLE_THR', '30')
    every_level(monkeypatch)
    cfg = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, rho=rho, freq=f, nPML=8, method='direct', rtol=1e-10)
    if seed % 2 == 0:
        fs = (True, False, False, False)
        cfg = dict(cfg, freeSurf=fs)
        cls = za.MiniZephyr
        ref = ho.DirectOperator(ho.minizephyr_coefficients(nz, nx, c, rho, f, dx=10., dz=10., nPML=8, freeSurf=fs)) * q
    else:
        cls = za.Eurus
        ref = ho.DirectOperator(ho.eurus_coefficients(nz, nx, c, rho, f, dx=10., dz=10., nPML=8)[0]) * q
    monkeypatch.setenv('HELM_ND_GATHER21', '1')
    op = cls(cfg)
    u = np.array(op * q)
    print('seed %d: against LU %.2e, worst relres %.2e' % (seed, nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert all(i['status'] == 0 and i['relres'] <= 1e-10 for i in op.lastInfo), op.lastInfo
    assert nrm(u, ref) <= 1e-7, (seed, nrm(u, ref))
    monkeypatch.setenv('HELM_ND_GATHER21', '0')
    op2 = cls(cfg)
    u2 = np.array(op2 * q)
    print('   gathered against built %.2e, bit for bit: %s' % (nrm(u, u2), np.array_equal(u, u2)))
    assert nrm(u, u2) <= 1e-9
    del op.factors, op2.factors


@pytest.mark.parametrize('Disc,nf', [('Eurus', 2), ('MiniZephyr', 4)])
def test_gathered_f21_of_operators_factored_together_matches_one_at_a_time_bit_for_bit(helm_lib, monkeypatch, Disc, nf):
    'set-up of test_fused_levels_of_operators_factored_together_match_one_at_a_time_bit_for_bit: the children of frequency kf lie interleaved, the planes travel per frequency'
    import zephyr_amd as za
    from zephyr_amd.models import marmousi_like
    every_level(monkeypatch)
    monkeypatch.setenv('HELM_ND_GATHER21', '1')
    n = 200
    fr, _ = gather_fronts(helm_lib, n, n, 8)
    assert len(fr) >= 200 and (fr[:, 10] > 64).any() and ((fr[:, 10] > 16) & (fr[:, 10] <= 64)).any()
    c = marmousi_like(n, n, 12.)
    cls = getattr(za, Disc)
    freqs = [4.0, 6.5, 9.0, 11.0][:nf]
    locs = np.stack([np.linspace(300., 2000., 70), np.full(70, 24.)], axis=1)
    base = dict(nx=n, nz=n, dx=12., dz=12., c=c, nPML=10, rtol=1e-10, method='direct')
    q = za.SparseKaiserSource(base)(locs)
    single = []
    for f in freqs:
        op = cls(dict(base, freq=f))
        op.prefactor()
        single.append(np.array(op * q))
        del op.factors
    ops = [cls(dict(base, freq=f)) for f in freqs]
    za.prefactor_many(ops)
    together = [np.array(op * q) for op in ops]
    for a, b, op in zip(single, together, ops):
        assert np.array_equal(a, b)
        assert all(i['status'] == 0 and i['relres'] <= 1e-10 for i in op.lastInfo)


def test_gathered_f21_on_a_transposed_handle(helm_lib, monkeypatch):
    'the 41 x 150 MiniZephyr case with free surfaces, transposed: path on against off, and against the LU of the transposed oracle matrix'
    import zephyr_amd as za
    cls, nz, nx, fs = CASES[2]
    assert_plan_covers_the_cases(helm_lib, nz, nx, 8)
    every_level(monkeypatch)
    monkeypatch.setenv('HELM_ND_GATHER21', '1')
    cfg, q, C = case_setup(cls, nz, nx, fs)
    cfg = dict(cfg, transposed=True)
    op = za.MiniZephyr(cfg)
    u = np.array(op * q)
    ref = ho.DirectOperator(ac.transpose_planes(C)) * q
    plain = ho.DirectOperator(C) * q
    assert nrm(plain, ref) > 1e-3                                          # (A^-T and A^-1 differ on this model)
    print('transposed: against LU %.2e, worst relres %.2e' % (nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert nrm(u, ref) <= 1e-8
    assert all(i['status'] == 0 and i['relres'] <= 1e-11 for i in op.lastInfo), op.lastInfo
    monkeypatch.setenv('HELM_ND_GATHER21', '0')
    op2 = za.MiniZephyr(cfg)
    u2 = np.array(op2 * q)
    assert np.array_equal(u, u2)
    del op.factors, op2.factors
