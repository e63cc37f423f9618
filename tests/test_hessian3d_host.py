"""CPU: the exact pseudo-Hessian diagonal and the (c, rho) blocks of a 3-D problem on the host -- the moments route of frechet3d.py against one-cell brute force
and an independent 27-colour evaluation, what each term of the formula is worth, the Gardner combination, the closed form of the velocity, a probe identity,
the interface of Helm3DProblem with hessian3D=True, what is refused with and without the key, and two gloo ranks (tests/hessian3d_cases.py has the bounds)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import zephyr_amd as za
from zephyr_amd import frechet, frechet3d
from tests import survey3d_cases as s3
from tests import survey3d_density_cases as d3c
from tests import hessian3d_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ['12x11x13', '18x16x20']
_PAIRS = {}
X = dict(kind='pseudoHessian', linearisation='full')


def pair(grid, mode='fixed', gardner=False):
    'one problem / survey pair per case for the whole module, with its solved fields: (prob, sv, [u^ per frequency], the host list of fields())'
    key = (grid, mode, gardner)
    if key not in _PAIRS:
        prob, sv = hc.host_pair(grid, mode, gardner)
        _PAIRS[key] = (prob, sv) + hc.fields_of(prob)
    return _PAIRS[key]


def small_op(dims, seed=0):
    return s3.OracleHelm3D(d3c.small_config(dims, seed))


def sample_cells(dims, n, seed=0):
    'the eight corners, the centre of every face, cells inside the absorbing layers and a random sample: boundary nodes and PML cells are in it'
    nz, ny, nx = dims
    idx = lambda z, y, x: (z * ny + y) * nx + x
    cells = {idx(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)}
    cells |= {idx(0, ny // 2, nx // 2), idx(nz - 1, ny // 2, nx // 2), idx(nz // 2, 0, nx // 2), idx(nz // 2, ny - 1, nx // 2), idx(nz // 2, ny // 2, 0),
              idx(nz // 2, ny // 2, nx - 1), idx(1, 1, 1), idx(1, ny // 2, 2), idx(nz - 2, ny - 2, nx - 2), idx(nz // 2, ny // 2, nx // 2)}
    rng = np.random.default_rng(seed)
    cells |= set(int(i) for i in rng.choice(nz * ny * nx, n, replace=False))
    return np.array(sorted(cells))


def all_routes(op, uh, g):
    "{'blocks' (3, N), 'rho', 'c', 'gardner'} by the moments route, with the majorants"
    val = dict(blocks=frechet3d.pseudoHessianBlocks3(op, uh), rho=frechet3d.pseudoHessianDiagonal3(op, uh, 'rho'), c=frechet3d.pseudoHessianDiagonal3(op, uh, 'c'),
               gardner=frechet3d.pseudoHessianDiagonal3(op, uh, 'c', g))
    maj = dict(blocks=frechet3d.pseudoHessianBlocks3(op, uh, magnitude=True), rho=frechet3d.pseudoHessianDiagonal3(op, uh, 'rho', magnitude=True),
               c=frechet3d.pseudoHessianDiagonal3(op, uh, 'c', magnitude=True), gardner=frechet3d.pseudoHessianDiagonal3(op, uh, 'c', g, magnitude=True))
    return val, maj


def brute_in_density_units(op, uh, cells, g):
    bf = hc.brute_force(op, uh, cells, g)
    rho = np.broadcast_to(np.asarray(op.rho, dtype=np.float64).ravel(), (op.nrow,))[cells]
    return dict(blocks=np.stack([bf['cc'], -bf['cb'] / rho ** 2, bf['bb'] / rho ** 4]), rho=bf['bb'] / rho ** 4, c=bf['cc'], gardner=bf['total'])


# ---- 1. the moments route against brute force and the colours -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', [(3, 3, 3), (5, 6, 7)], ids=lambda d: 'x'.join(map(str, d)))
def test_small_grids_every_cell_against_one_cell_brute_force(dims):
    op = small_op(dims)
    N = op.nrow
    uh = s3.randc(np.random.default_rng(1), (N, 3))
    g = frechet3d.gardnerChain3(op)
    val, maj = all_routes(op, uh, g)
    cells = np.arange(N)
    bf = brute_in_density_units(op, uh, cells, g)
    w = {n: hc.worst(np.abs(val[n] - bf[n]), hc.host_bound(3, maj[n])) for n in val}
    col = dict(blocks=frechet3d.pseudoHessianColours3(op, uh, 'blocks'), rho=frechet3d.pseudoHessianColours3(op, uh, 'rho'),
               c=frechet3d.pseudoHessianColours3(op, uh, 'c'), gardner=frechet3d.pseudoHessianColours3(op, uh, 'c', g))
    wc = {n: hc.worst(np.abs(val[n] - col[n]), hc.host_bound(3, maj[n])) for n in val}
    coh = val['blocks'][1] / np.sqrt(val['blocks'][0] * val['blocks'][2])
    print('%s: worst error / bound against brute force %s, against the colours %s; coherence %.2f .. %.2f; min H_rhorho %.2e'
          % (dims, {n: '%.3f' % v for n, v in w.items()}, {n: '%.3f' % v for n, v in wc.items()}, coh.min(), coh.max(), val['rho'].min()))
    assert max(w.values()) <= 1.0 and max(wc.values()) <= 1.0
    assert np.all(val['rho'] > 0) and np.all(val['c'] > 0) and np.all(val['gardner'] > 0)          # boundary nodes included: they are columns of interior rows


@pytest.mark.parametrize('grid', GRIDS)
def test_oracle_pairs_against_the_colours_everywhere_and_brute_force_on_a_sample(grid):
    prob, sv, UH, _ = pair(grid)
    pg, _, UG, _ = pair(grid, gardner=True)
    dims = s3.HOST_GRIDS[grid][0]
    cells = sample_cells(dims, 40)
    for (p, U, names) in ((prob, UH, ('blocks', 'rho', 'c')), (pg, UG, ('gardner',))):
        op, uh = p.system.subProblems[0], U[0]
        g = frechet3d.gardnerChain3(op)
        k = uh.shape[1]
        val, maj = all_routes(op, uh, g)
        bf = brute_in_density_units(op, uh, cells, g)
        for n in names:
            col = frechet3d.pseudoHessianColours3(op, uh, 'blocks' if n == 'blocks' else ('rho' if n == 'rho' else 'c'), g if n == 'gardner' else None)
            wc = hc.worst(np.abs(val[n] - col), hc.host_bound(k, maj[n]))
            wb = hc.worst(np.abs(val[n][..., cells] - bf[n]), hc.host_bound(k, maj[n][..., cells]))
            print('%s %s: worst error / bound against the colours (every cell) %.3f, against brute force (%d cells) %.3f' % (grid, n, wc, len(cells), wb))
            assert wc <= 1.0 and wb <= 1.0


@pytest.mark.parametrize('variant', [dict(tables='row'), dict(rows='centre'), dict(mask=False)], ids=lambda v: '%s=%s' % next(iter(v.items())))
def test_leaving_a_term_out_misses_by_many_bounds(variant):
    "L in the place of its column entries, only the row of the cell itself, the interior mask of the neighbour rows left out: each misses the colours by > 100 bounds"
    prob, sv, UH, _ = pair('12x11x13')
    op, uh = prob.system.subProblems[0], UH[0]
    g = frechet3d.gardnerChain3(op)
    k = uh.shape[1]
    _, maj = all_routes(op, uh, g)
    got = dict(blocks=frechet3d.pseudoHessianBlocks3(op, uh, **variant), rho=frechet3d.pseudoHessianDiagonal3(op, uh, 'rho', **variant),
               gardner=frechet3d.pseudoHessianDiagonal3(op, uh, 'c', g, **variant))
    col = dict(blocks=frechet3d.pseudoHessianColours3(op, uh, 'blocks'), rho=frechet3d.pseudoHessianColours3(op, uh, 'rho'), gardner=frechet3d.pseudoHessianColours3(op, uh, 'c', g))
    w = {n: hc.worst(np.abs(got[n] - col[n]), hc.host_bound(k, maj[n])) for n in got}
    w['cross'] = hc.worst(np.abs(got['blocks'][1] - col['blocks'][1]), hc.host_bound(k, maj['blocks'][1]))
    print('%s: worst error / bound %s' % (variant, {n: '%.3g' % v for n, v in w.items()}))
    assert min(w.values()) >= 100.0, w


# ---- 2. blocks, Gardner, the closed form, the probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid,mode', [('12x11x13', 'fixed'), ('12x11x13', 'relative'), ('18x16x20', 'fixed')])
def test_block_rows_are_the_two_diagonals_and_a_gram_matrix(grid, mode):
    prob, sv, UH, F = pair(grid, mode)
    B = prob.hessianBlocks(None, u=F, **X)
    Hc, Hr = prob.illumination(None, u=F, parameter='c', **X), prob.illumination(None, u=F, parameter='rho', **X)
    assert B.shape == (3, prob.nrow) and B.dtype == np.float64 and Hc.shape == (prob.nrow,) and Hc.dtype == np.float64
    assert s3.rel(B[0], Hc) <= 1e-14 and s3.rel(B[2], Hr) <= 1e-14
    inside = frechet3d.interiorMask3(s3.HOST_GRIDS[grid][0])          # (a solved field is zero on the boundary nodes: identity rows)
    assert np.all(B[0] >= 0) and np.all(B[2] >= 0) and np.all(B[0][inside] > 0) and np.all(B[2][inside] > 0)
    assert np.all(B[1] ** 2 <= B[0] * B[2] * (1 + 1e-12))
    coh = B[1][inside] / np.sqrt(B[0][inside] * B[2][inside])
    print('%s %s: coherence of the blocks %.3f .. %.3f' % (grid, mode, coh.min(), coh.max()))
    assert np.abs(coh).max() > 0.1                           # the cross entry is not small
    # 'operator' and 'full' are the same derivative with an explicit rho
    assert np.array_equal(prob.hessianBlocks(None, u=F, kind='pseudoHessian', linearisation='operator'), B)
    assert np.array_equal(prob.illumination(None, u=F, kind='pseudoHessian', linearisation='operator', parameter='rho'), Hr)
    # and blockSolve takes them
    r = s3.randc(np.random.default_rng(5), sv.nD)
    gj = prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full', parameter='joint')
    z = frechet.blockSolve(B, gj, damping=1e-3)
    assert z.shape == gj.shape and np.all(np.isfinite(z))


@pytest.mark.parametrize('grid', GRIDS)
def test_gardner_total_is_the_combination_of_the_blocks_at_the_default_density(grid):
    "H_total = H_cc + 2 g H_cb + g^2 H_bb of the same model given as an explicit rho = 310 Re(c)^0.25; in (c, rho) units g H_cb = rho' H_crho, rho' = d rho / d c"
    pg, sg, UG, FG = pair(grid, gardner=True)
    c = np.asarray(pg.systemConfig['c'])
    pe, se = hc.host_pair(grid, rho=frechet3d.GARDNER_FACTOR * c.real ** frechet3d.GARDNER_POWER)
    Ht = pg.illumination(None, u=FG, perFreq=True, **X)
    st = complex(pg.system.scaleTerm)
    for i, uh in enumerate(UG):
        op = pe.system.subProblems[i]
        assert np.array_equal(np.asarray(op.rho), np.asarray(pg.system.subProblems[i].rho))
        rho = np.asarray(op.rho, dtype=np.float64).ravel()
        dr = -rho ** 2 * frechet3d.gardnerChain3(op)
        B, M = frechet3d.pseudoHessianBlocks3(op, uh), frechet3d.pseudoHessianBlocks3(op, uh, magnitude=True)
        want = B[0] + 2 * dr * B[1] + dr ** 2 * B[2]
        maj = M[0] + 2 * np.abs(dr) * M[1] + dr ** 2 * M[2]
        w = hc.worst(np.abs(Ht[i] / abs(st) ** 2 - want), 2 * hc.host_bound(uh.shape[1], maj))
        print('%s f%d: Gardner diagonal against the combination of the blocks, worst error / bound %.3f' % (grid, i, w))
        assert w <= 1.0


@pytest.mark.parametrize('grid', GRIDS)
def test_velocity_with_an_explicit_density_is_the_closed_form(grid):
    prob, sv, UH, F = pair(grid)
    Hc, E = prob.illumination(None, u=F, perFreq=True, parameter='c', **X), prob.illumination(None, u=F, kind='energy', perFreq=True)
    for i in range(sv.nfreq):
        W = frechet3d.velocityPseudoHessianWeight3(prob.system.subProblems[i])
        assert np.abs(Hc[i] - W * E[i]).max() <= 64 * s3.U53 * np.abs(Hc[i]).max() and np.all(np.abs(Hc[i] - W * E[i]) <= 64 * s3.U53 * Hc[i])


@pytest.mark.parametrize('grid', GRIDS)
def test_probe_identity_on_one_colour(grid):
    "a random +-1 vector on one colour: the columns have disjoint supports, so sum_s ||dA[v] u^_s||^2 is the sum of H over the cells of the colour"
    prob, sv, UH, _ = pair(grid)
    pg, _, UG, _ = pair(grid, gardner=True)
    dims = s3.HOST_GRIDS[grid][0]
    iz, iy, ix = (a.ravel() for a in np.mgrid[0:dims[0], 0:dims[1], 0:dims[2]])
    rng = np.random.default_rng(8)
    for colour in ((0, 0, 0), (1, 2, 0), (2, 1, 2)):
        ind = (iz % 3 == colour[0]) & (iy % 3 == colour[1]) & (ix % 3 == colour[2])
        v = np.where(ind, rng.choice([-1., 1.], ind.size), 0.)
        op, uh = prob.system.subProblems[0], UH[0]
        og, ug = pg.system.subProblems[0], UG[0]
        g = frechet3d.gardnerChain3(og)
        k = uh.shape[1]
        cases = dict(rho=(frechet3d.buoyancySources3(op, frechet3d.densityChain3(op) * v, uh), op, uh, 'rho', None),
                     c=(frechet3d.bornSources3(op, v, uh), op, uh, 'c', None),
                     gardner=(frechet3d.bornSources3(og, v, ug) + frechet3d.buoyancySources3(og, g * v, ug), og, ug, 'c', g))
        for n, (q, o, u, par, ch) in cases.items():
            H, M = frechet3d.pseudoHessianDiagonal3(o, u, par, ch), frechet3d.pseudoHessianDiagonal3(o, u, par, ch, magnitude=True)
            lhs, rhs = (abs(q) ** 2).sum(), H[ind].sum()
            assert abs(lhs - rhs) <= hc.host_bound(k, M[ind].sum()), (grid, colour, n, lhs, rhs)


# ---- 3. the interface -----------------------------------------------------------------------------------------------------------------------------------------
def test_routes_per_frequency_rows_and_a_model_dict():
    prob, sv, UH, F = pair('12x11x13')
    N = prob.nrow
    for call, kw, shape in ((prob.illumination, dict(parameter='rho', **X), (N,)), (prob.illumination, dict(parameter='c', **X), (N,)), (prob.hessianBlocks, X, (3, N))):
        total, rows = call(None, u=F, **kw), call(None, u=F, perFreq=True, **kw)
        assert total.shape == shape and rows.shape == (sv.nfreq,) + shape and s3.rel(rows.sum(axis=0), total) <= 1e-15
        assert s3.rel(call(None, **kw), total) <= 1e-13                       # u=None: solved, used, dropped
        m = dict(c=np.array(prob.systemConfig['c']), rho=np.array(prob.systemConfig['rho']))
        assert np.array_equal(call(m, u=F, **kw), total)
    pg, sg, UG, FG = pair('12x11x13', gardner=True)
    Hg = pg.illumination(None, u=FG, **X)
    assert Hg.shape == (N,) and np.all(Hg >= 0) and Hg.max() > 0 and s3.rel(pg.illumination(None, **X), Hg) <= 1e-13
    # the value: |st|^2 sum_f of the host maps
    st = complex(prob.system.scaleTerm)
    want = sum(abs(st) ** 2 * frechet3d.pseudoHessianDiagonal3(prob.system.subProblems[i], UH[i], 'rho') for i in range(sv.nfreq))
    assert s3.rel(prob.illumination(None, u=F, parameter='rho', **X), want) <= 1e-15
    # the 'c' diagonal with an explicit rho needs the new key alone
    sc = dict(prob.systemConfig)
    del sc['derivatives3D']
    p1, s1 = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    p1.pair(s1)
    assert np.array_equal(p1.illumination(None, u=F, parameter='c', **X), prob.illumination(None, u=F, parameter='c', **X))
    for call in (lambda: p1.illumination(None, u=F, parameter='rho', **X), lambda: p1.hessianBlocks(None, u=F, **X)):
        with pytest.raises(NotImplementedError, match='needs derivatives3D=True beside hessian3D=True'):
            call()


def test_refusals_with_the_key_say_why():
    prob, sv, UH, F = pair('12x11x13')
    pg, sg, UG, FG = pair('12x11x13', gardner=True)
    with pytest.raises(NotImplementedError, match=r'(?s)illumination\(kind=\'gaussNewton\'\).*nrec back-solves'):
        prob.illumination(None, u=F, kind='gaussNewton', linearisation='full')
    with pytest.raises(NotImplementedError, match=r'(?s)hessianBlocks\(kind=\'gaussNewton\'\).*nrec back-solves'):
        prob.hessianBlocks(None, u=F)                                       # (the default kind)
    with pytest.raises(NotImplementedError, match=r'(?s)side=\'receiver\'.*source-side'):
        prob.illumination(None, side='receiver', **X)
    with pytest.raises(NotImplementedError, match=r'(?s)side=\'receiver\'.*source-side'):
        prob.hessianBlocks(None, side='receiver', **X)
    for par in ('Q', 'cQ'):
        with pytest.raises(NotImplementedError, match=r'(?s)parameter=%r.*\(c, Q\)' % (par,)):
            prob.illumination(None, u=F, parameter=par, **X)
    with pytest.raises(ValueError, match=r'(?s)parameter=\'joint\'.*hessianBlocks'):
        prob.illumination(None, u=F, parameter='joint', **X)
    with pytest.raises(NotImplementedError, match=r'(?s)hessianBlocks needs an explicit `rho`.*Gardner'):
        pg.hessianBlocks(None, u=FG, **X)
    for kw in (dict(linearisation='operator'), dict(linearisation='full', parameter='rho')):
        with pytest.raises(NotImplementedError, match=r"(?s)without `rho`.*linearisation='full', parameter='c'.*Gardner"):
            pg.illumination(None, u=FG, kind='pseudoHessian', **kw)
    with pytest.raises(ValueError, match="needs linearisation='operator'"):
        prob.illumination(None, u=F, kind='pseudoHessian', linearisation='scaler', parameter='rho')
    with pytest.raises(ValueError, match='has no linearisation'):
        prob.illumination(None, u=F, kind='energy', linearisation='full')
    with pytest.raises(ValueError, match='kind is'):
        prob.hessianBlocks(None, u=F, kind='energy')
    p64, s64 = hc.host_pair('12x11x13', fieldsDtype='complex64')
    with pytest.raises(NotImplementedError, match=r'(?s)complex128 store.*complex64'):
        p64.illumination(None, **X)
    with pytest.raises(NotImplementedError, match=r'(?s)complex128 store.*complex64'):
        p64.hessianBlocks(None, **X)


def test_without_the_key_every_refusal_of_today_is_still_raised():
    for make in (s3.host_pair, d3c.host_pair):                              # (no key at all; derivatives3D alone)
        prob, sv = make('12x11x13')
        for kw in (dict(linearisation='full'), dict(linearisation='operator', parameter='rho'), dict(kind='gaussNewton'), dict(parameter='rho'),
                   dict(kind='energy', linearisation='full')):
            with pytest.raises(NotImplementedError, match=r'(?s)illumination\(kind=.*is not built for 3-D problems.*derivative planes of the 2-D operators.*\'scaler\' are served'):
                prob.illumination(None, **kw)
    prob, sv = s3.host_pair('12x11x13')
    with pytest.raises(NotImplementedError, match='no density derivative in 3-D'):
        prob.hessianBlocks(None, kind='pseudoHessian', linearisation='full')
    prob, sv = d3c.host_pair('12x11x13')
    with pytest.raises(NotImplementedError, match=r'(?s)hessianBlocks.*Hvec\(parameter=\'joint\'\)'):
        prob.hessianBlocks(None, kind='pseudoHessian', linearisation='full')
    with pytest.raises(NotImplementedError, match=r'(?s)hessianBlocks.*Hvec\(parameter=\'joint\'\)'):
        prob.hessianBlocks(anything=1)


def test_the_scaler_kinds_return_the_same_bits_with_and_without_the_key():
    prob, sv, UH, F = pair('12x11x13')
    plain, sp_ = s3.host_pair('12x11x13')
    Fp = plain.fields(None)
    for kw in (dict(kind='energy'), dict(kind='pseudoHessian'), dict(kind='energy', perFreq=True), dict(kind='pseudoHessian', side='receiver')):
        a = plain.illumination(None, **kw) if 'side' in kw else plain.illumination(None, u=Fp, **kw)
        b = prob.illumination(None, **kw) if 'side' in kw else prob.illumination(None, u=F, **kw)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    before = prob.illumination(None, u=F, kind='pseudoHessian')
    prob.illumination(None, u=F, parameter='rho', **X)
    prob.hessianBlocks(None, u=F, **X)
    assert np.array_equal(prob.illumination(None, u=F, kind='pseudoHessian').view(np.uint64), before.view(np.uint64))


def test_the_library_interface_names_the_new_entry_points():
    from zephyr_amd import _lib
    assert {'helm_ph3_coefficients_device', 'helm_ph3_moments_accumulate_device'} <= set(_lib.exported_symbols())


# ---- 4. two ranks -------------------------------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import survey3d_cases as s3
from tests import hessian3d_cases as hc
ok = True
ref, _ = hc.host_pair('12x11x13', shardFreqs=False)
prob, sv = hc.host_pair('12x11x13')
assert prob.ownedFreqs == [dist.get_rank()] and ref.ownedFreqs == [0, 1]
X = dict(kind='pseudoHessian', linearisation='full')
for call, rcall, kw, shape in ((prob.illumination, ref.illumination, dict(parameter='rho', **X), (2, prob.nrow)), (prob.illumination, ref.illumination, dict(parameter='c', **X), (2, prob.nrow)),
                               (prob.hessianBlocks, ref.hessianBlocks, X, (2, 3, prob.nrow))):
    rows = call(None, perFreq=True, **kw)                    # (the row of the other rank's frequency arrives through the all-reduce)
    ok = ok and rows.shape == shape and s3.rel(rows, rcall(None, perFreq=True, **kw)) < 1e-12
    ok = ok and s3.rel(call(None, u=ref.fields(None), **kw), rows.sum(axis=0)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'the two frequencies sharded over two ranks: one all-reduce gives every rank the single-rank diagonal and blocks'
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29677', WORLD_SIZE='2', PYTHONPATH=ROOT, OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
