"""CPU, on the oracle doubles: illumination(kind='gaussNewton') is the diagonal of the operator that Hvec applies -- every cell of a 13 x 17 survey and about 36
cells of the 37 x 53 one against e_i . Hvec(e_i), an independent brute force through a sparse LU of the transposed matrix, the radius of two lags, frechet.lagGram
against the diagonals of U U^H, the 80-bit references of the two device kernels and what they reject, the interface, what is refused, and two gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import gaussnewton_cases as gc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10          # per cell and relative: the tolerance of the host identities of test_full_host.py
GN = dict(kind='gaussNewton')


# ---- 1. the definition, every cell ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [False, True], ids=['mz', 'hd'])
@pytest.mark.parametrize('variant', sorted(gc.VARIANTS))
def test_every_cell_of_the_small_survey_is_the_diagonal_of_hvec(variant, hd):
    """13 x 17, nPML = 3, a fixed array, three frequencies (one damped): D[i] against e_i . Hvec(e_i) for all 221 cells, per cell and relative; a cell where Hvec
    gives exactly 0 gives exactly 0"""
    lin, par, density = gc.VARIANTS[variant]
    prob, sv = gc.small_pair(hd, density)
    assert (complex(prob.system.scaleTerm).imag != 0) == hd
    uF = prob.fields()
    D = prob.illumination(u=uF, linearisation=lin, parameter=par, **GN)
    assert D.shape == (prob.nrow,) and D.dtype == np.float64 and np.all(D >= 0) and prob.nrow == 221
    cells = list(range(prob.nrow))
    want = gc.hvec_diagonal(prob, uF, cells, linearisation=lin, parameter=par)
    worst = gc.rel(D, want)
    print('%s hd=%s: worst |D[i] - e_i.Hvec(e_i)| / |.| over %d cells %.2e (%d exact zeros, values %.1e .. %.1e)' % (
        variant, hd, len(cells), worst, int((want == 0).sum()), want[want > 0].min(), want.max()))
    assert worst <= TOL


# ---- 2. the 37 x 53 case -------------------------------------------------------------------------------------------------------------------------------------
BIG = [('full', 'c', True, False), ('full', 'c', False, True), ('operator', 'rho', True, True), ('operator', 'c', True, False)]


@pytest.fixture(scope='module')
def solved():
    "(hd, density) -> the 37 x 53 pair with its host fields, solved once and left unchanged"
    out = {}
    for hd, density in ((False, True), (True, False), (True, True)):
        prob, sv = xc.pair('fixed', hd, density)
        out[(hd, density)] = dict(prob=prob, sv=sv, uF=prob.fields())
    return out


@pytest.mark.parametrize('lin,par,density,hd', BIG, ids=['%s-%s-%s-%s' % (a, b, 'rho' if c else 'gardner', 'hd' if d else 'mz') for a, b, c, d in BIG])
def test_sampled_cells_of_the_37x53_case_against_hvec_and_the_brute_force(solved, lin, par, density, hd):
    """corners, boundary lines, cells next to them, every absorbing layer, under the free surface and the interior: D[i] against e_i . Hvec(e_i) and against
    sum_s sum_r |g_r^T (E_i u^_s)|^2 with E_i u^ by applyPlanes and g_r from a sparse LU of the transposed oracle matrix"""
    s = solved[(hd, density)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    cells = gc.cells_37x53()
    assert len(cells) == len(set(cells)) == 36
    D = prob.illumination(u=uF, linearisation=lin, parameter=par, **GN)
    want = gc.hvec_diagonal(prob, uF, cells, linearisation=lin, parameter=par)
    brute = gc.brute_force(prob, sv, uF, cells, prob._resolveLinearisation(lin, par, 'illumination'), par)
    e1, e2 = gc.rel(D[cells], want), gc.rel(D[cells], brute)
    print('%s %s: worst relative difference to Hvec %.2e, to the brute force %.2e (values %.1e .. %.1e)' % (lin, par, e1, e2, want[want > 0].min(), want.max()))
    assert e1 <= TOL and e2 <= TOL and np.all(D >= 0)


def test_not_proportional_to_the_pseudo_hessian(solved):
    "the ratio to illumination(linearisation='full') varies by more than 3 over 25 interior cells: Shin's diagonal leaves the receiver side out"
    s = solved[(False, True)]
    prob, uF = s['prob'], s['uF']
    cells = gc.interior_cells_25()
    ratio = prob.illumination(u=uF, linearisation='full', **GN)[cells] / prob.illumination(u=uF, linearisation='full')[cells]
    print('gaussNewton / pseudoHessian over %d interior cells: max / min = %.1f' % (len(cells), ratio.max() / ratio.min()))
    assert ratio.max() / ratio.min() > 3.0


# ---- 3. the radius ------------------------------------------------------------------------------------------------------------------------------------------
def test_lags_up_to_two_carry_the_trace_and_lags_up_to_one_do_not():
    "Gamma and Phi from full outer products: masked to lags <= 2 the trace is the unmasked one, masked to lags <= 1 it is not"
    sc, op, _ = pc.operator('tile', 'explicit')
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    u, g = pc.columns(N, 3, seed=1), pc.columns(N, 2, seed=2)
    E = fr.blockCoefficients(nz, nx, lambda v: fr.velocityPlanes(op, v))

    def blocks(a, radius):
        G = a @ np.conj(a).T
        iz, ix = np.divmod(np.arange(N), nx)
        B = np.zeros((N, 9, 9), dtype=np.complex128)
        for p, (pz, px) in enumerate(fr.LAGS):
            for q, (qz, qx) in enumerate(fr.LAGS):
                if max(abs(qz - pz), abs(qx - px)) > radius:
                    continue
                ok = (iz + pz >= 0) & (iz + pz < nz) & (ix + px >= 0) & (ix + px < nx) & (iz + qz >= 0) & (iz + qz < nz) & (ix + qx >= 0) & (ix + qx < nx)
                i = np.arange(N)[ok]
                B[i, p, q] = G[i + pz * nx + px, i + qz * nx + qx]
        return B
    full = fr.gaussNewtonTrace(E, blocks(g, 9), blocks(u, 9))
    two = fr.gaussNewtonTrace(E, blocks(g, 2), blocks(u, 2))
    one = fr.gaussNewtonTrace(E, blocks(g, 1), blocks(u, 1))
    assert np.array_equal(full, two) and full.max() > 0
    assert gc.rel(one[full > 0], full[full > 0]) > 1e-3
    # and the planes of lagGram are those blocks
    assert ac.rel(fr._gramBlocks(fr.lagGram(u, nz, nx), nz, nx), blocks(u, 2)) <= 1e-15


# ---- 4. lagGram -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dc.KERNEL_CASES, ids=['%dx%dx%d' % c for c in dc.KERNEL_CASES])
def test_lag_gram_is_u_uh_along_its_diagonals(case):
    "13 stored planes and the 12 conjugates against the 25 diagonals of U U^H; 3 x 3 and 33 x 3: lag 2 leaves the grid"
    nz, nx, nsrc = case
    U, _ = gc.gram_inputs(nz, nx, nsrc, seed=nz + nx)
    C = fr.lagGram(U.T, nz, nx)
    assert C.shape == (13, nz * nx) and len(fr.GRAM_LAGS) == 13
    diag = gc.gram_from_outer(U, nz, nx)
    touched = gc.gram_touched(nz, nx)
    scale = np.abs(U).max() ** 2
    for l, (dz, dx) in enumerate(fr.GRAM_LAGS):
        assert np.max(np.abs(C[l] - diag[(dz, dx)])) <= 1e-13 * scale and np.all(C[l][~touched[l]] == 0)
        mirrored = np.conj(fr._at(C[l].reshape((nz, nx)), -dz, -dx)).ravel()                     # the lag (-dz, -dx), read at the shifted cell
        assert np.max(np.abs(mirrored - diag[(-dz, -dx)])) <= 1e-13 * scale
    if nx == 3:
        assert touched[2].sum() == nz and touched[7].sum() == nz - 1                              # (0, 2) and (1, 2): one pair per row on three columns


# ---- 5. the references of the device kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(4, 4, 4), (5, 61, 5), (33, 3, 5)], ids=['4x4x4', '5x61x5', '33x3x5'])
def test_gram_reference_bounds_plain_fp64_and_rejects_wrong_pairings(case):
    nz, nx, nsrc = case
    U, C0 = gc.gram_inputs(nz, nx, nsrc, seed=3)
    ref, mag, _ = gc.gram_reference(C0, U, nz, nx)
    bound = gc.c_gram(nsrc) * gc.U64 * mag
    plain = C0 + fr.lagGram(U.T, nz, nx)
    assert dc.worst_ratio(plain, ref, bound) <= 1.0
    assert dc.worst_ratio(C0 + np.conj(fr.lagGram(U.T, nz, nx)), ref, bound) > 1e6                # the conjugate on the wrong side
    shifted = fr.lagGram(U.T, nz, nx)[[1, 0] + list(range(2, 13))]
    assert dc.worst_ratio(C0 + shifted, ref, bound) > 1e6                                         # planes paired with the wrong lag


@pytest.mark.parametrize('mode', sorted(gc.GN_MODES))
def test_combine_reference_bounds_plain_fp64_and_rejects_wrong_evaluations(mode):
    lin, par, density = gc.GN_MODES[mode]
    sc, op, _ = pc.operator('tile', 'explicit' if density else 'gardner')
    chain = None if density else fr.gardnerChain(sc['c'])
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    Cu, Cg, _ = gc.combine_inputs(nz, nx, seed=4)
    W = np.random.default_rng(2).uniform(0.5, 2.0, N)
    H0 = np.zeros(N)
    ref, mag = gc.combine_reference(op, Cu, Cg, mode, chain, 0.37, W, H0)
    bound = gc.C_GN * gc.U64 * mag
    assert np.all(ref >= 0) and ref.max() > 0
    plain = gc.combine_reference(op, Cu, Cg, mode, chain, 0.37, W, H0, dtype=np.complex128)[0]
    assert gc.worst_ratio(plain, ref, bound) <= 1.0
    if mode == 'diagonal':
        return
    wrong = {'Gamma and Phi exchanged': gc.combine_reference(op, Cg, Cu, mode, chain, 0.37, W, H0, dtype=np.complex128)[0],
             'planes paired with the wrong lag': gc.combine_reference(op, Cu, Cg[[0, 2, 1] + list(range(3, 13))], mode, chain, 0.37, W, H0, dtype=np.complex128)[0]}
    if mode != 'mass':          # (the mass term alone has one column and real weights per row: it sees Phi[i, i] and the real part of Gamma)
        wrong['one set conjugated'] = gc.combine_reference(op, np.conj(Cu), Cg, mode, chain, 0.37, W, H0, dtype=np.complex128)[0]
        kw = dict(parameter=par, chain=chain)
        u = np.random.default_rng(4)          # the pseudo-Hessian of columns with these planes' zero lag is another quantity
        wrong['the pseudo-Hessian'] = 0.37 * W * fr.pseudoHessianDiagonal(op, ac.randc(u, (N, 3)), **kw)
    for what, H in wrong.items():
        assert gc.worst_ratio(H, ref, bound) > 1e3, what


# ---- 6. the interface ---------------------------------------------------------------------------------------------------------------------------------------
def test_rows_sum_to_the_total_and_u_none_solves_the_fields(solved):
    s = solved[(True, True)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    for kw in (dict(linearisation='full'), dict(linearisation='operator', parameter='rho'), dict(linearisation='operator'), dict()):
        H = prob.illumination(u=uF, **GN, **kw)
        rows = prob.illumination(u=uF, perFreq=True, **GN, **kw)
        assert rows.shape == (sv.nfreq, prob.nrow) and np.all(rows >= 0) and ac.rel(rows.sum(axis=0), H) <= 1e-15
        assert ac.rel(prob.illumination(**GN, **kw), H) <= 1e-12
    assert np.array_equal(prob.illumination(u=uF, linearisation='full', parameter='rho', **GN), prob.illumination(u=uF, linearisation='operator', parameter='rho', **GN))


def test_value_errors(solved):
    prob, uF = solved[(True, True)]['prob'], solved[(True, True)]['uF']
    with pytest.raises(ValueError, match='side'):
        prob.illumination(side='receiver', **GN)
    with pytest.raises(ValueError, match="'gaussNewton'"):
        prob.illumination(u=uF, kind='gaussnewton')
    with pytest.raises(ValueError):
        prob.illumination(u=uF, parameter='rho', **GN)
    moving, _ = xc.pair('relative', False)
    with pytest.raises(ValueError, match='fixed receiver arrays'):
        moving.illumination(**GN)


def test_refusals_carry_the_messages_of_the_born_data(solved):
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

    def messages(prob, **kw):
        out = []
        for call in (lambda: prob.illumination(**GN, **kw), lambda: prob.JvecBorn(None, np.ones(prob.nrow), **kw)):
            with pytest.raises(NotImplementedError) as ei:
                call()
            out.append(str(ei.value))
        return out
    for prob in (prob25, probv, probe, probm):
        with pytest.raises(NotImplementedError):          # every linearisation of this kind, 'scaler' included
            prob.illumination(**GN)
        for lin in ('operator', 'full'):
            mine, born = messages(prob, linearisation=lin)
            if prob is probm:          # (JvecBorn refuses a multiscale survey before it resolves the linearisation: the same sentence without the keyword)
                born = born.replace('JvecBorn ', 'JvecBorn(linearisation=%r) ' % lin)
            assert len(mine) > 20 and mine.replace('illumination(', 'JvecBorn(') == born
    g = solved[(True, False)]['prob']                                             # no `rho` in the config
    for kw in (dict(linearisation='operator'), dict(linearisation='full', parameter='rho'), dict(linearisation='operator', parameter='rho')):
        mine, born = messages(g, **kw)
        assert 'rho' in mine and mine.replace('illumination(', 'JvecBorn(') == born


# ---- 7. two ranks -----------------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests import full_cases as xc
ok = True
GN = dict(kind='gaussNewton')
for density, kws in ((True, (dict(linearisation='full'), dict(linearisation='operator', parameter='rho'), dict())), (False, (dict(linearisation='full'),))):
    ref, _ = xc.pair('fixed', True, density=density, shardFreqs=False)
    prob, sv = xc.pair('fixed', True, density=density)
    assert prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
    for kw in kws:
        rows = prob.illumination(perFreq=True, **GN, **kw)                     # (rows of the other rank's frequencies arrive through the all-reduce)
        ok = ok and rows.shape == (3, prob.nrow) and ac.rel(rows, ref.illumination(perFreq=True, **GN, **kw)) < 1e-12
        ok = ok and ac.rel(prob.illumination(u=ref.fields(), **GN, **kw), rows.sum(axis=0)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'frequencies sharded over two ranks: the one existing all-reduce gives every rank the single-rank result, per-frequency rows included'
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29647', WORLD_SIZE='2', PYTHONPATH=ROOT, OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
