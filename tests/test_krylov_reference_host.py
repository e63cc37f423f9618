"""CPU: the references of tests/krylov_cases.py, which tests/test_gpu_krylov.py holds the Krylov drivers of csrc/krylov.hip to.

1. they are right: run to rtol = 1e-10 in extended precision they reach the sparse-LU solution of the oracle's matrix;
2. sensitivity: d_k = ||x_k^double - x_k^exact|| / ||x_k^exact|| per case, column and k -- what the tolerance of the GPU file is made of;
3. teeth: every mutated recurrence misses x_k^exact by at least 1000 x 16 max(d_k, 64 u), from k = 2 on (the omega mutant from k = 1), on every case and
   every non-zero column.  That is a condition on the INPUTS of krylov_cases: a case that fails it gets other inputs, never another factor.

4. the refinement round: on case 'R' the double reference says which columns meet the scaled criterion with the unscaled residual still above rtol.

The planes are the oracle's here; on the GPU they are the handle's own."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import helm3d_oracle as h3
from oracle import helm_oracle as ho
from tests import krylov_cases as kc

pytestmark = pytest.mark.skipif(not kc.have_x87(), reason='numpy.longdouble is not the 80-bit format here')

TEETH = 1000.0


@functools.lru_cache(maxsize=None)
def planes(name):
    return kc.system_planes(name, kc.oracle_planes(name))


def columns(name):
    Q, kinds = kc.rhs_columns(name, max(kc.case_ncols(name)))
    keep = [j for j, k in enumerate(kinds) if k != 'zero']
    return Q[keep], [kinds[j] for j in keep]


@functools.lru_cache(maxsize=None)
def sensitivity(name, method, ipm):
    Q, _ = columns(name)
    return kc.sensitivity(name, planes(name), Q, kc.PREMULS[ipm], method, max(kc.case_ks(name)))


def case_method_pairs(names):
    return [(n, m) for n in names for m in kc.case_methods(n)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,method', case_method_pairs(('S', 'M', 'TTI', '3S')))
def test_exact_reference_reaches_the_sparse_lu_solution(name, method):
    """one complex normal column, premul = 0.3 - 1.7j, to ||r|| <= 1e-10 ||bbar|| of the scaled recurrence: within 1e-7 of the LU solution, the bound at which
    the suite holds the device's own Krylov solves to sparse LU"""
    C0 = kc.oracle_planes(name)
    kind = kc.CASES[name]['kind']
    A = ho.eurus_matrix(C0) if kind == 'tti' else (h3.coefficients_to_csr3(C0) if kind == '3d' else ho.coefficients_to_csr(C0))
    Q, _ = kc.rhs_columns(name, 1)
    pm = kc.PREMULS[1]
    x_lu = spla.splu(A.tocsc(), permc_spec='MMD_ATA' if kind == '3d' else None).solve(pm * Q[0])
    x, its = kc.ITERATES[method](kc.System(name, planes(name), kc.CLD), Q, pm, 50000, rtol=1e-10)
    err = kc.relnorm(x, x_lu[None])[0]
    print('%s %s: %d iterations, %.2e from sparse LU' % (name, method, its, err))
    assert its < 50000
    assert err <= 1e-7


def test_sweeps_are_the_oracles():
    "the slicing sweeps against the oracle's matrices, forward and adjoint, 2-D, 3-D and the 2 x 2 block system"
    rng = np.random.default_rng(5)
    for name in ('S', 'TTI', '3S'):
        C0 = kc.oracle_planes(name)
        kind = kc.CASES[name]['kind']
        A = ho.eurus_matrix(C0) if kind == 'tti' else (h3.coefficients_to_csr3(C0) if kind == '3d' else ho.coefficients_to_csr(C0))
        S = kc.System(name, planes(name), np.complex128)
        X = rng.standard_normal((2, kc.rows_of(name))) + 1j * rng.standard_normal((2, kc.rows_of(name)))
        Xs = X.reshape((2,) + S.vshape)
        for adjoint, M in ((False, A), (True, A.conj().T)):
            want = (M @ X.T).T
            got = S.apply(Xs, adjoint=adjoint, raw=True).reshape(2, -1)
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the row equilibration: every row of the scaled coupled system has unit 2-norm
    S = kc.System('TTI', planes('TTI'), kc.CLD)
    n2 = (np.abs(S.Abar) ** 2).reshape(2, 2, 9, -1).sum(axis=(1, 2))
    assert np.abs(n2 - 1).max() <= 1e-17


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,method', case_method_pairs(kc.ITERATE_CASES))
def test_sensitivity_table(name, method):
    """d_k of every column and k; the first iterate is a handful of roundings away from the exact one (the 64 u floor of the GPU tolerance covers it) and no d_k
    comes near the mutants' misses (test_teeth holds that by the factor)"""
    for ipm in (0, 1):
        _, d = sensitivity(name, method, ipm)
        print('%s %s premul %s  d_k: %s' % (name, method, kc.PREMULS[ipm], '  '.join('k=%d %.1e..%.1e' % (k, d[k - 1].min(), d[k - 1].max()) for k in kc.case_ks(name))))
        assert np.all(np.isfinite(d)) and np.all(d > 0)
        assert d[0].max() <= 64 * kc.U


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,method', case_method_pairs(kc.ITERATE_CASES))
def test_teeth(name, method):
    for ipm in (0, 1):
        ex, d = sensitivity(name, method, ipm)
        Q, kinds = columns(name)
        S = kc.System(name, planes(name), kc.CLD)
        for mutant in kc.MUTANTS[method]:
            mu = kc.ITERATES[method](S, Q, kc.PREMULS[ipm], max(kc.case_ks(name)), mutant=mutant)
            first = 1 if mutant in ('omega_st', 'z_forward') else 2
            worst = np.inf
            for k in kc.case_ks(name):
                if k < first:
                    continue
                miss = kc.relnorm(mu[k - 1], ex[k - 1])
                need = TEETH * kc.MARGIN * np.maximum(d[k - 1], 64 * kc.U)
                worst = min(worst, float((miss / need).min()))
                assert np.all(miss >= need), (name, method, mutant, k, miss, need)
            print('%s %s premul %s %s: misses by at least %.1e x the required 1000 x tolerance' % (name, method, kc.PREMULS[ipm], mutant, worst))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_restart_case_splits_its_batch():
    """solve_block_krylov stops its first round at ||r|| <= rtol / 2 ||bbar|| of the scaled system and refines the columns whose unscaled residual is still above
    rtol.  On case 'R' at rtol = 1e-3 the point source on the smallest diagonal entry is above by more than a factor of two, the point source in the middle of
    the grid below by more than a factor of two: what tests/test_gpu_krylov.py then asks of the device does not hang on a rounding."""
    C = planes('R')
    Q, kinds = kc.restart_columns(C)
    ratios = {j: kc.refinement_ratio('R', C, Q[j], kc.RESTART_RTOL) for j in (0, 1, 3, 4)}
    print('unscaled residual / rtol after the first round (iterations): %s' % '  '.join('column %d %.2f (%d)' % (j, r, it) for j, (r, it) in ratios.items()))
    assert ratios[3][0] > 2 and ratios[1][0] < 0.5
