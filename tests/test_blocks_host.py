"""CPU, on the oracle doubles: hessianBlocks gives the 2 x 2 diagonal blocks of the operator that Hvec(parameter='joint') applies -- every cell of the 13 x 17
survey and 36 cells of the 37 x 53 one against both cross entries of Hvec, the single-parameter diagonals and a brute force through a sparse LU of the
transposed matrix; the pseudo-Hessian blocks against their one-cell brute force and as the Gauss-Newton blocks with Gamma = I; the polarisation identity against
the chain of the existing diagonals; the 80-bit references of the two device kernels and what they reject; the interface, what is refused, blockSolve, and
two gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import blocks_cases as bc
from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import gaussnewton_cases as gc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10          # per cell: the tolerance of tests/test_gaussnewton_host.py; rows 0 and 2 relative to the value, row 1 to sqrt(B0 B2) of the cell
LINS = ('full', 'operator')


# ---- 1. the definition, every cell ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [False, True], ids=['mz', 'hd'])
@pytest.mark.parametrize('lin', LINS)
def test_every_cell_of_the_small_survey_is_the_block_of_hvec(lin, hd):
    """13 x 17, a fixed array, three frequencies: B[1] against Hvec([0; e_i])[i] and Hvec([e_i; 0])[N + i] for all 221 cells on the scale sqrt(B0 B2) of the cell,
    rows 0 and 2 against the single-parameter diagonals; exact zeros stay exact; every block is a Gram matrix; the coherence is large somewhere, in both signs"""
    prob, sv = gc.small_pair(hd)
    uF = prob.fields()
    B = prob.hessianBlocks(u=uF, kind='gaussNewton', linearisation=lin)
    assert B.shape == (3, prob.nrow) and B.dtype == np.float64 and prob.nrow == 221
    cells = list(range(prob.nrow))
    a, b = bc.hvec_cross(prob, uF, cells, lin)
    scale = np.sqrt(B[0] * B[2])
    e1, e2 = bc.cross_error(B[1], a, scale), bc.cross_error(B[1], b, scale)
    d0 = gc.rel(B[0], prob.illumination(u=uF, kind='gaussNewton', linearisation=lin, parameter='c'))
    d2 = gc.rel(B[2], prob.illumination(u=uF, kind='gaussNewton', linearisation=lin, parameter='rho'))
    coh = bc.coherence(B)
    print('%s hd=%s: cross entry against Hvec %.2e / %.2e of sqrt(B0 B2), rows 0 / 2 against the diagonals %.2e / %.2e, coherence %.3f .. %.3f, %d exact zeros' % (
        lin, hd, e1, e2, d0, d2, coh.min(), coh.max(), int((a == 0).sum())))
    assert e1 <= TOL and e2 <= TOL and d0 <= TOL and d2 <= TOL
    assert bc.gram_properties(B)
    assert np.any((B[0] == 0) & (B[2] > 0))                        # (boundary cells: H_cc = 0, H_rhorho > 0, and the cross entry exactly 0)
    assert np.abs(coh).max() > 0.5 and coh.max() > 0 > coh.min()          # (the test cannot pass on a vanishing cross term)


# ---- 2. the 37 x 53 case -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def solved():
    "hd -> the 37 x 53 pair with an explicit density and its host fields, solved once and left unchanged"
    out = {}
    for hd in (False, True):
        prob, sv = xc.pair('fixed', hd, True)
        out[hd] = dict(prob=prob, sv=sv, uF=prob.fields())
    return out


@pytest.mark.parametrize('lin,hd', [('full', False), ('full', True), ('operator', True), ('operator', False)])
def test_sampled_cells_of_the_37x53_case_against_hvec_and_the_brute_force(solved, lin, hd):
    "the 36 cells of gaussnewton_cases.cells_37x53: the three rows against Hvec and against the brute force through a sparse LU of the transposed oracle matrix"
    s = solved[hd]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    cells = gc.cells_37x53()
    B = prob.hessianBlocks(u=uF, linearisation=lin)
    Bc = B[:, cells]
    scale = np.sqrt(Bc[0] * Bc[2])
    a, b = bc.hvec_cross(prob, uF, cells, lin)
    brute = bc.brute_force(prob, sv, uF, cells, lin)
    errs = [bc.cross_error(Bc[1], a, scale), bc.cross_error(Bc[1], b, scale), bc.cross_error(Bc[1], brute[1], scale), gc.rel(Bc[0], brute[0]), gc.rel(Bc[2], brute[2]),
            gc.rel(Bc[0], gc.hvec_diagonal(prob, uF, cells, linearisation=lin, parameter='c'))]
    print('%s hd=%s: cross against Hvec %.2e / %.2e, against the brute force %.2e; rows 0 / 2 against the brute force %.2e / %.2e, row 0 against Hvec %.2e' % ((lin, hd) + tuple(errs)))
    assert max(errs) <= TOL and bc.gram_properties(B)


# ---- 3. the pseudo-Hessian blocks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin', LINS)
@pytest.mark.parametrize('name', ['tiny', 'tile'])
def test_pseudo_hessian_blocks_against_the_one_cell_brute_force_and_gamma_identity(name, lin):
    sc, op, _ = pc.operator(name, 'explicit')
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    u = pc.columns(N, 3, seed=5)
    B = fr.pseudoHessianBlocks(op, u, lin)
    cells = pc.sample_cells(nz, nx, sc['nPML'])
    brute = bc.ph_brute_force(op, u, lin, cells)
    Bc = B[:, cells]
    scale = np.sqrt(Bc[0] * Bc[2])
    assert gc.rel(Bc[0], brute[0]) <= TOL and gc.rel(Bc[2], brute[2]) <= TOL and bc.cross_error(Bc[1], brute[1], scale) <= TOL
    assert bc.gram_properties(B) and np.abs(bc.coherence(B)).max() > 0.1
    # Gamma = I: the Gram planes of the N unit columns
    G = fr.gaussNewtonBlocks(op, fr.lagGram(u, nz, nx), fr.lagGram(np.eye(N), nz, nx), lin)
    full = np.sqrt(B[0] * B[2])
    assert gc.rel(G[0], B[0]) <= TOL and gc.rel(G[2], B[2]) <= TOL and bc.cross_error(G[1], B[1], full) <= TOL


def test_pseudo_hessian_rows_are_the_single_parameter_diagonals(solved):
    prob, uF = solved[True]['prob'], solved[True]['uF']
    for lin in LINS:
        B = prob.hessianBlocks(u=uF, kind='pseudoHessian', linearisation=lin)
        assert gc.rel(B[0], prob.illumination(u=uF, linearisation=lin, parameter='c')) <= TOL
        assert gc.rel(B[2], prob.illumination(u=uF, linearisation=lin, parameter='rho')) <= TOL
        assert bc.gram_properties(B)


# ---- 4. polarisation --------------------------------------------------------------------------------------------------------------------------------------------
def test_polarisation_against_the_chain_of_the_existing_diagonals():
    "with a chain t the existing diagonals are those of E^c + t E^b: cc + 2 t cb + t^2 bb of the (c, b)-unit blocks, t of the size of sqrt(cc / bb)"
    sc, op, _ = pc.operator('tile', 'explicit')
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    rng = np.random.default_rng(6)
    u, g = pc.columns(N, 3, seed=7), pc.columns(N, 4, seed=8)
    Cu, Cg = fr.lagGram(u, nz, nx), fr.lagGram(g, nz, nx)
    for B, diag in ((fr.gaussNewtonBlocks(op, Cu, Cg, 'full'), lambda t: fr.gaussNewtonDiagonal(op, Cu, Cg, 'c', chain=t)),
                    (fr.pseudoHessianBlocks(op, u, 'full'), lambda t: fr.pseudoHessianDiagonal(op, u, 'c', chain=t))):
        cc, cb, bb = bc.unit_blocks(op, B)
        size = np.sqrt(np.where(bb > 0, cc / np.where(bb > 0, bb, 1), 0))
        t = np.where(size > 0, size, np.median(size[size > 0])) * rng.uniform(0.5, 2.0, N) * rng.choice([-1.0, 1.0], N)
        want = cc + 2 * t * cb + t * t * bb
        scale = cc + 2 * np.abs(t * cb) + t * t * bb
        got = diag(t)
        err = float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1)))
        assert err <= TOL and np.all(got[scale == 0] == 0)
        assert np.max(np.abs(2 * t * cb) / np.where(scale > 0, scale, 1)) > 0.1          # (the cross term is part of the sum, not noise)


# ---- 5. the references of the device kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin', LINS)
def test_gn_reference_bounds_plain_fp64_and_rejects_wrong_evaluations(lin):
    sc, op, _ = pc.operator('tile', 'explicit')
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    Cu, Cg, _ = gc.combine_inputs(nz, nx, seed=4)
    H0 = np.zeros((3, N))
    ref, mag = bc.gn_reference(op, Cu, Cg, lin, 0.37, H0)
    bound = bc.C_GNB * bc.U64 * mag
    assert np.all(ref[0] >= 0) and np.all(ref[2] >= 0) and np.any(ref[1] > 0) and np.any(ref[1] < 0)
    plain = bc.gn_reference(op, Cu, Cg, lin, 0.37, H0, dtype=np.complex128)[0]
    assert max(bc.worst_rows(plain, ref, bound)) <= 1.0
    assert max(bc.worst_rows(0.37 * bc.gn_wrong(op, Cu, Cg, lin, None), ref, bound)) <= 1.0
    for how in ('conjugate', 'own_row', 'sign', 'gamma_transposed'):
        worst = bc.worst_rows(0.37 * bc.gn_wrong(op, Cu, Cg, lin, how), ref, bound)
        assert max(worst) > 1e3, (how, worst)


@pytest.mark.parametrize('lin', LINS)
def test_ph_reference_bounds_plain_fp64_and_rejects_wrong_evaluations(lin):
    sc, op, _ = pc.operator('tile', 'explicit')
    N = sc['nz'] * sc['nx']
    nsrc = 5
    u = pc.columns(N, nsrc, seed=9)
    H0 = np.zeros((3, N))
    ref, mag, _ = bc.ph_reference(op, u, lin, 0.37, H0)
    bound = bc.c_phb(nsrc) * bc.U64 * mag
    assert np.any(ref[1] > 0) and np.any(ref[1] < 0)
    plain = bc.ph_reference(op, u, lin, 0.37, H0, dtype=np.complex128)[0]
    assert max(bc.worst_rows(plain, ref, bound)) <= 1.0
    assert max(bc.worst_rows(0.37 * bc.ph_wrong(op, u, lin, None), ref, bound)) <= 1.0
    for how in ('conjugate', 'own_row', 'sign'):
        worst = bc.worst_rows(0.37 * bc.ph_wrong(op, u, lin, how), ref, bound)
        assert worst[1] > 1e3 and worst[0] <= 1.0 and worst[2] <= 1.0, (how, worst)


# ---- 6. the interface ---------------------------------------------------------------------------------------------------------------------------------------
def test_rows_sum_to_the_total_and_u_none_solves_the_fields(solved):
    s = solved[True]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    for kw in (dict(kind='gaussNewton', linearisation='full'), dict(kind='gaussNewton', linearisation='operator'), dict(kind='pseudoHessian', linearisation='full'),
               dict(kind='pseudoHessian', linearisation='operator')):
        B = prob.hessianBlocks(u=uF, **kw)
        rows = prob.hessianBlocks(u=uF, perFreq=True, **kw)
        assert rows.shape == (sv.nfreq, 3, prob.nrow) and ac.rel(rows.sum(axis=0), B) <= 1e-15
        assert ac.rel(prob.hessianBlocks(**kw), B) <= 1e-12
    assert np.array_equal(prob.hessianBlocks(u=uF), prob.hessianBlocks(u=uF, kind='gaussNewton', linearisation='full'))          # the defaults
    R = prob.hessianBlocks(kind='pseudoHessian', side='receiver')
    assert R.shape == (3, prob.nrow) and bc.gram_properties(R) and gc.rel(R[0], prob.illumination(side='receiver', linearisation='full')) <= TOL
    moving, _ = xc.pair('relative', False)
    M = moving.hessianBlocks(kind='pseudoHessian')
    assert bc.gram_properties(M) and gc.rel(M[2], moving.illumination(linearisation='full', parameter='rho')) <= TOL


def test_value_errors(solved):
    prob, uF = solved[True]['prob'], solved[True]['uF']
    with pytest.raises(ValueError, match='joint'):
        prob.hessianBlocks(u=uF, linearisation='scaler')
    with pytest.raises(ValueError, match='linearisation'):
        prob.hessianBlocks(u=uF, linearisation='exact')
    with pytest.raises(ValueError, match='kind'):
        prob.hessianBlocks(u=uF, kind='energy')
    with pytest.raises(ValueError, match='kind'):
        prob.hessianBlocks(u=uF, kind='gaussnewton')
    with pytest.raises(ValueError, match='side'):
        prob.hessianBlocks(kind='gaussNewton', side='receiver')
    with pytest.raises(ValueError, match='side'):
        prob.hessianBlocks(kind='pseudoHessian', side='both')
    with pytest.raises(ValueError, match='u must be None'):
        prob.hessianBlocks(u=uF, kind='pseudoHessian', side='receiver')
    moving, _ = xc.pair('relative', False)
    with pytest.raises(ValueError, match='fixed receiver arrays'):
        moving.hessianBlocks()
    with pytest.raises(ValueError, match='fixed receiver arrays'):
        moving.hessianBlocks(kind='pseudoHessian', side='receiver')
    with pytest.raises(ValueError):          # (an existing test holds illumination to this; the blocks are a method of their own)
        prob.illumination(u=uF, parameter='joint', linearisation='full')


def test_refusals_carry_the_messages_of_hvec():
    import zephyr_amd as za
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    prob25, sv25 = ac.host_pair('25d-fixed', rho=2000.)
    scv = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True, Q=50.)
    probv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    probv.pair(svv)
    sce = fc.config('fixed', False, Disc=za.Eurus, hostGradient=True)
    probe, sve = Helm2DProblem(sce), Helm2DSurvey(sce)
    probe.pair(sve)
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq, rho=2000.)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    gardner, _ = xc.pair('fixed', True, False)

    def message(call):
        with pytest.raises(NotImplementedError) as ei:
            call()
        return str(ei.value)
    for prob in (prob25, probv, probe, probm, gardner):
        for lin in LINS:
            for kind in ('gaussNewton', 'pseudoHessian'):
                mine = message(lambda: prob.hessianBlocks(kind=kind, linearisation=lin))
                resolved = message(lambda: prob._resolveLinearisation(lin, 'joint', 'hessianBlocks'))
                assert len(mine) > 20 and mine == resolved and mine.startswith('hessianBlocks(linearisation=%r)' % lin)
    assert 'rho' in message(lambda: gardner.hessianBlocks())


def test_block_solve():
    rng = np.random.default_rng(3)
    N = 50
    a, b = rng.normal(size=(2, N)), rng.normal(size=(2, N))
    B = np.stack([(a * a).sum(0), (a * b).sum(0), (b * b).sum(0)])
    B[:, :3] = 0.0                                                  # exactly zero blocks
    B[0, 3], B[1, 3] = 0.0, 0.0                                     # H_cc = 0, H_rhorho > 0
    g = rng.normal(size=2 * N)
    lam = 1e-3
    z = fr.blockSolve(B, g, lam)
    assert z.shape == (2 * N,) and z.dtype == np.float64
    lc, lr = lam * B[0].max(), lam * B[2].max()
    for i in range(N):
        want = np.linalg.solve(np.array([[B[0, i] + lc, B[1, i]], [B[1, i], B[2, i] + lr]]), np.array([g[i], g[N + i]]))
        assert np.allclose([z[i], z[N + i]], want, rtol=1e-12, atol=0)
    D = B.copy()
    D[1] = 0.0
    zd = fr.blockSolve(D, g, lam)
    assert np.allclose(zd[:N], g[:N] / (D[0] + lam * D[0].max()), rtol=1e-14, atol=0) and np.allclose(zd[N:], g[N:] / (D[2] + lam * D[2].max()), rtol=1e-14, atol=0)
    for bad in (0.0, -1e-3, np.nan, np.inf, None, np.ones(2)):
        with pytest.raises((ValueError, TypeError)):
            fr.blockSolve(B, g, bad)
    for Bb, gb in ((B[:2], g), (B.ravel(), g), (B, g[:-1]), (B, g.reshape((2, N))), (B[None], g)):
        with pytest.raises(ValueError):
            fr.blockSolve(Bb, gb, lam)


# ---- 7. two ranks -----------------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests import full_cases as xc
ok = True
ref, _ = xc.pair('fixed', True, shardFreqs=False)
prob, sv = xc.pair('fixed', True)
assert prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
for kw in (dict(kind='gaussNewton', linearisation='full'), dict(kind='pseudoHessian', linearisation='operator')):
    rows = prob.hessianBlocks(perFreq=True, **kw)                     # (rows of the other rank's frequencies arrive through the all-reduce)
    ok = ok and rows.shape == (3, 3, prob.nrow) and ac.rel(rows, ref.hessianBlocks(perFreq=True, **kw)) < 1e-12
    ok = ok and ac.rel(prob.hessianBlocks(u=ref.fields(), **kw), rows.sum(axis=0)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'frequencies sharded over two ranks: one all-reduce of the (nfreq, 3, N) array gives every rank the single-rank result'
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29653', WORLD_SIZE='2', PYTHONPATH=ROOT, OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
