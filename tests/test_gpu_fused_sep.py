"""GPU: the small separator levels of the factorisation in one kernel per level (k_sep_factor_small, nd_leaf.hip; HELM_ND_FUSEDSEP) -- against the sparse LU of
the oracle's matrix and against the batched path it replaces, on grids whose plans (checked here, on the host) hold separator fronts of 3-8 and of 9-16
cells, fronts padded below their group's size, fronts on the grid's edge with short rings, and both leaf and separator children; with dozens of fronts
flagged and re-eliminated; for several operators in the same launches; and on a transposed handle.  HELM_ND_FUSEDSEP_MIN=1 forces the path: by default
only levels of several hundred fronts take it, which the small grids of this suite never have."""
import ctypes

import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


def nrm(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def fused_fronts(lib, nz, nx, leaf):
    'rows {z0, z1, x0, x1, cut, pos, s, m, kid0, kid1, smax, mmax} of the fronts the fused kernel takes, and the whole plan (helm_direct_plan: host only)'
    n = lib.helm_direct_plan(nz, nx, leaf, None, 0)
    plan = np.zeros((n, 12), dtype=np.int32)
    assert lib.helm_direct_plan(nz, nx, leaf, plan.ctypes.data_as(P), n) == n
    take = (plan[:, 4] >= 0) & (plan[:, 10] <= 16) & (plan[:, 10] + plan[:, 11] <= 128) & (plan[:, 11] > 0)
    return plan[take], plan


def assert_plan_covers_the_cases(lib, nz, nx, leaf):
    small, plan = fused_fronts(lib, nz, nx, leaf)
    assert len(small) >= 20
    assert (small[:, 6] < small[:, 10]).any()                              # fronts padded below smax
    assert (small[:, 7] < small[:, 11]).any()                              # short rings: fronts on the grid's edge
    assert any(plan[r[8], 4] < 0 for r in small) and any(plan[r[8], 4] >= 0 for r in small)      # leaf children and separator children
    if leaf == 8:
        assert (small[:, 10] > 8).any()                                    # the 16-wide kernel
    else:
        assert (small[:, 10] <= 8).any() and small[:, 6].min() <= 4        # the 8-wide kernel, separators of 3-4 cells
    return small


CASES = [('MiniZephyr', 64, 64, (0, 0, 0, 0)), ('Eurus', 70, 90, (0, 0, 0, 0)), ('MiniZephyr', 41, 150, (1, 0, 0, 1)),
         ('Eurus', 128, 128, (0, 0, 0, 0)), ('MiniZephyr', 57, 33, (0, 1, 1, 0))]


def case_setup(cls, nz, nx, fs):
    'model, sources and oracle planes of test_fused_leaf_level_matches_sparse_lu'
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


@pytest.mark.parametrize('leaf', [8, 4])
@pytest.mark.parametrize('cls,nz,nx,fs', CASES)
def test_fused_separator_levels_match_sparse_lu_and_the_batched_path(helm_lib, monkeypatch, cls, nz, nx, fs, leaf):
    import zephyr_amd as za
    assert_plan_covers_the_cases(helm_lib, nz, nx, leaf)
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '1')
    monkeypatch.setenv('HELM_ND_LEAF', str(leaf))
    cfg, q, C = case_setup(cls, nz, nx, fs)
    op = getattr(za, cls)(cfg)
    u = np.array(op * q)
    ref = ho.DirectOperator(C, eurus=(cls == 'Eurus')) * q
    print('%s %dx%d leaf %d: against LU %.2e, worst relres %.2e' % (cls, nz, nx, leaf, nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert nrm(u, ref) <= 1e-8
    assert all(i['status'] == 0 and i['relres'] <= 1e-11 for i in op.lastInfo), op.lastInfo
    monkeypatch.setenv('HELM_ND_FUSEDSEP', '0')
    op2 = getattr(za, cls)(cfg)
    u2 = np.array(op2 * q)
    print('   fused against batched %.2e, bit for bit: %s' % (nrm(u, u2), np.array_equal(u, u2)))
    assert nrm(u, u2) <= 1e-9
    del op.factors, op2.factors


@pytest.mark.parametrize('seed', [0, 1])
def test_fused_levels_with_dozens_of_fronts_flagged_and_reeliminated(helm_lib, monkeypatch, seed):
    """grid and sources of test_lu_treatment_forced_on_many_fronts (seed 0: MiniZephyr with a free surface, seed 1: Eurus) with the threshold at 30: the
    estimates the fused kernel forms flag dozens of its fronts, which stabilise_group rebuilds from the children and eliminates again"""
    import zephyr_amd as za
    rng = np.random.default_rng(77 + seed)
    nz, nx = int(rng.integers(150, 260)), int(rng.integers(150, 300))
    c = 1600. + 2200. * rng.random((nz, nx))
    rho = 1000. + 600. * rng.random((nz, nx))
    f = float(rng.uniform(8., 20.))
    nrhs = int(rng.integers(3, 40))
    q = np.zeros((nz * nx, nrhs), complex)
    q[rng.integers(0, nz * nx, nrhs), np.arange(nrhs)] = rng.standard_normal(nrhs) + 1j * rng.standard_normal(nrhs)
    small, _ = fused_fronts(helm_lib, nz, nx, 8)
    assert len(small) >= 200 and (small[:, 10] <= 8).any() and (small[:, 10] > 8).any()
    monkeypatch.setenv('HELM_ND_STABLE_THR', '30')
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '1')
    cfg = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, rho=rho, freq=f, nPML=8, method='direct', rtol=1e-10)
    if seed % 2 == 0:
        fs = (True, False, False, False)
        cfg = dict(cfg, freeSurf=fs)
        cls = za.MiniZephyr
        ref = ho.DirectOperator(ho.minizephyr_coefficients(nz, nx, c, rho, f, dx=10., dz=10., nPML=8, freeSurf=fs)) * q
    else:
        cls = za.Eurus
        ref = ho.DirectOperator(ho.eurus_coefficients(nz, nx, c, rho, f, dx=10., dz=10., nPML=8)[0]) * q
    op = cls(cfg)
    u = np.array(op * q)
    print('seed %d: against LU %.2e, worst relres %.2e' % (seed, nrm(u, ref), max(i['relres'] for i in op.lastInfo)))
    assert all(i['status'] == 0 and i['relres'] <= 1e-10 for i in op.lastInfo), op.lastInfo
    assert nrm(u, ref) <= 1e-7, (seed, nrm(u, ref))
    monkeypatch.setenv('HELM_ND_FUSEDSEP', '0')
    op2 = cls(cfg)
    u2 = np.array(op2 * q)
    print('   fused against batched %.2e' % nrm(u, u2))
    assert nrm(u, u2) <= 1e-9
    del op.factors, op2.factors


@pytest.mark.parametrize('Disc,nf', [('Eurus', 2), ('MiniZephyr', 4)])
def test_fused_levels_of_operators_factored_together_match_one_at_a_time_bit_for_bit(helm_lib, monkeypatch, Disc, nf):
    'set-up of test_operators_factored_in_the_same_launches_match_one_at_a_time_bit_for_bit: the kernel does the same arithmetic per (front, frequency) whatever nf is'
    import zephyr_amd as za
    from zephyr_amd.models import marmousi_like
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '1')
    n = 200
    small, _ = fused_fronts(helm_lib, n, n, 8)
    assert len(small) >= 200 and (small[:, 10] <= 8).any() and (small[:, 10] > 8).any()
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


def test_fused_levels_on_a_transposed_handle(helm_lib, monkeypatch):
    'the 41 x 150 MiniZephyr case with free surfaces, transposed (the tr form of the condition estimate): path on against off, and against the LU of the transposed oracle matrix'
    import zephyr_amd as za
    cls, nz, nx, fs = CASES[2]
    assert_plan_covers_the_cases(helm_lib, nz, nx, 8)
    monkeypatch.setenv('HELM_ND_FUSEDSEP_MIN', '1')
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
    monkeypatch.setenv('HELM_ND_FUSEDSEP', '0')
    op2 = za.MiniZephyr(cfg)
    u2 = np.array(op2 * q)
    print('   fused against batched %.2e' % nrm(u, u2))
    assert nrm(u, u2) <= 1e-9
    del op.factors, op2.factors
