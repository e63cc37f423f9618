"""GPU: the judge of the direct path -- the true-residual kernels k_resid_nm<4> / k_resid_nm_lds<4, 1> with their reduction, and the node-major plumbing
around them (zephyr_amd/csrc/nd_resid.hip) -- against q' - A x in numpy.clongdouble with A from the oracle, through the test hook helm_debug_nm_stage,
which goes through the launchers the solver calls (nd_resid_nm + helm_launch_fin_ex as true_residual_norms does, nd_prep_transpose_norm, nd_pack_cols ...).

The bounds are derived in tests/resid_cases.py (u = 2^-53): the stored residual within 24 u S of the reference element by element (28 with the scaled q'),
Uout within 4 u |oscale| |x| (the same bits when oscale = 1), ||r||^2 within (2 N + 8) u of the sum over what was stored, or, when nothing is stored,
| sqrt(rr) - ||r_ref|| | <= ||24 u S|| + (N + 4) u ||r_ref||, and ||q'||^2 to (2 N + 8) u relative.  tests/test_resid_reference.py shows that a plain fp64
evaluation meets them.  Every test prints the worst ratio |out - ref| / bound it saw.

Two data regimes: x and q independent (the residual is O(1): a dropped tap, a skipped cell or a wrong column is O(1) against 1e-15), and q = fl(A x) (the
residual cancels to rounding: only the componentwise bound means anything).

Every input lies in a buffer with NaN between the rows (ld > ncol) and in one row past the end; every output buffer is filled with a sentinel first.  Padding
and the columns nobody owns come back bit for bit, Q comes back bit for bit unless the residual is stored over it, and no interior element of a written
output keeps its sentinel.

Not covered here: the rhs-major residual epilogue of k_stencil_t and the coupled-system path direct_batch_sys2, the 3-D kernels, k_axpy_one, and the
decision logic of direct_batch_nm itself (refine_done, minority_above), which a real solve reaches (tests/test_gpu_direct.py); a solve steered into the
minority pass would need fault injection in the solve path, the kernels of that pass are run here in its order instead."""
import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import resid_cases as rc
from tests.zgemm_shapes import U, crand

pytestmark = pytest.mark.gpu
SENT, NAN = rc.SENT, rc.NAN
PADS = (1, 3, 61)
CAPS = (1, 3, 0)                   # 0: the solver's own value


@pytest.fixture(autouse=True)
def _x87():
    if not rc.have_x87():
        pytest.skip('numpy.longdouble is not the 80-bit x87 format on this host: no extended-precision reference')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def padded(values, ld, fill, cols=None):
    """(rows + 1) x ld buffer of `fill` with `values` (rows x n) in the columns `cols` (default: the first n)"""
    rows, n = values.shape
    buf = np.full((rows + 1, ld), fill, dtype=np.complex128)
    buf[:rows, (slice(0, n) if cols is None else cols)] = values
    return buf


def interior_only(buf, before, rows, cols):
    """everything but buf[:rows, cols] has the bits it had; nothing inside kept the sentinel"""
    a, b = buf.copy(), before.copy()
    a[:rows, cols], b[:rows, cols] = 0, 0
    assert np.array_equal(bits(a), bits(b)), 'the launch wrote outside its output'
    assert not np.any(buf[:rows, cols] == SENT), 'an interior element kept its sentinel'


def shape_of(nz, nx, ncol):
    """(lanes, row groups, tiles, launches) nd_resid_nm documents for a batch of ncol columns on an (nz, nx) grid"""
    lanes = 64 if ncol <= 64 else (128 if ncol <= 128 else 256)
    return lanes, 256 // lanes, ((nz + 3) // 4) * ((nx + 31) // 32), (ncol + 255) // 256


def check_report(rep, nz, nx, ncol, cap):
    lanes, groups, tiles, launches = shape_of(nz, nx, ncol)
    assert (rep[0], rep[1], rep[3], rep[4]) == (lanes, groups, launches, tiles), rep
    most = min((tiles + groups - 1) // groups, 2048)
    assert rep[2] == max(1, min(most, cap)) if cap else 1 <= rep[2] <= most, rep


def run_resid(lib, C, x, q, ref, cap=0, store=None, qnorm=0, qmap=None, pad=0, uout=False, oscale=1 + 0j, xin_is_u=0, qmask=None, q_in=None, expect=0):
    """one RESID call on padded buffers and every check of it.  x: what the launch reads (u when xin_is_u); store: None, 'rout', 'inplace'; q_in: what Q holds
    (q with NaN where the mask says it is not read); returns ({quantity: ratio}, report, rr, qq)"""
    _, nz, nx = C.shape
    N, ncol = x.shape
    p1, p2, p3 = PADS[pad % 3], PADS[(pad + 1) % 3], PADS[(pad + 2) % 3]
    ldq = ncol + p2
    cols = np.arange(ncol) if qmap is None else qmap.astype(np.int64)
    Xb = padded(x, ncol + p1, NAN)
    Qb = padded(q if q_in is None else q_in, ldq, NAN, cols)
    Rb = np.full((N + 1, ldq), SENT) if store == 'rout' else None
    Ub = np.full((N + 1, ncol + p3), SENT) if uout else None
    Q0 = Qb.copy()
    rcode, rep, rr, qq = rc.nm_stage(lib, rc.RESID, nz=nz, nx=nx, ncol=ncol, nblk_cap=cap, planes=np.ascontiguousarray(C).ravel(), Xin=Xb.ravel(), ldin=ncol + p1,
                                     Q=Qb.ravel(), ldq=ldq, qmap=None if qmap is None else qmap.astype(np.int32), store=1 if store else 0, qnorm=qnorm,
                                     Rout=None if Rb is None else Rb.ravel(), Uout=None if Ub is None else Ub.ravel(), ldu=ncol + p3, oscale=oscale,
                                     qmask=qmask, xin_is_u=xin_is_u)
    assert rcode == expect, (rcode, expect)
    if expect:
        assert np.array_equal(bits(Qb), bits(Q0)) and (Rb is None or np.all(Rb == SENT)) and (Ub is None or np.all(Ub == SENT)), 'a refused call wrote'
        return {}, rep, rr, qq
    check_report(rep, nz, nx, ncol, cap)
    out = {}
    r = None
    if store == 'inplace':
        interior_only(Qb, Q0, N, cols)
        r = Qb[:N, cols]
    else:
        assert np.array_equal(bits(Qb), bits(Q0)), 'Q changed although the residual was not stored over it'
        if store == 'rout':
            interior_only(Rb, np.full_like(Rb, SENT), N, cols)
            r = Rb[:N, cols]
    if r is not None:
        out['stored'] = rc.ratio_stored(r, ref)
        out['rr_stored'] = rc.ratio_rr_stored(rr, r)
    else:
        out['rr_norms'] = rc.ratio_rr_norms(rr, ref)
    if qnorm:
        out['qq'] = rc.ratio_qq(qq, ref)
    else:
        assert np.all(np.isnan(qq)), 'qq written without qnorm'
    if uout:
        interior_only(Ub, np.full_like(Ub, SENT), N, np.arange(ncol))
        out['uout'] = rc.ratio_uout(Ub[:N, :ncol], ref, oscale)
    return out, rep, rr, qq


class Worst(dict):
    def add(self, ratios, what):
        for k, v in ratios.items():
            assert v <= 1.0, (what, k, v)
            self[k] = max(self.get(k, 0.0), v)

    def show(self, what):
        print('%s: worst |out - ref| / bound  %s' % (what, '  '.join('%s %.4f' % kv for kv in sorted(self.items()))))
        assert self and all(v <= 1.0 for v in self.values()), what


# ---- 1. norms and stored residual on every grid and width ---------------------------------------------------------------------------------------------------
def widths(nz, nx):
    """every width on the grids of a few hundred cells and below; on the larger ones the widths at which the launch changes (lanes, chunks) and the two ends"""
    return rc.NCOLS if nz * nx <= 400 else [1, 64, 65, 128, 129, 256, 257, 513]


STORES = (None, 'rout', 'inplace')


@pytest.mark.parametrize('nz,nx', rc.GRIDS, ids=['%dx%d' % g for g in rc.GRIDS])
def test_norms_and_stored_residual(helm_lib, nz, nx):
    """every width x both regimes x the three store modes: a launch that stores nothing, one that stores r to Rout and one that stores it over Q (no map: Q
    itself moves on by 256 columns from chunk to chunk); with and without ||q||^2, the cap on the partial sums, the paddings and the discretisation cycling
    with the case so that every store mode meets every cap and both values of qnorm"""
    worst, n, seen = Worst(), 0, set()
    for i, ncol in enumerate(widths(nz, nx)):
        kind = rc.kind_for(nz, nx, i)
        for regime in ('random', 'cancel'):
            C, x, q = rc.operands(kind, nz, nx, ncol, regime)
            ref = rc.Ref(C, x, q)
            for s, store in enumerate(STORES):
                k = n // 3 + s                                   # (n // 3: the case; + s: the mode of a case meets another cap and qnorm than its neighbour)
                cap, qnorm = CAPS[k % 3], (k // 3 + s) % 2
                ratios, rep, _, _ = run_resid(helm_lib, C, x, q, ref, cap=cap, store=store, qnorm=qnorm, pad=k)
                worst.add(ratios, (nz, nx, ncol, kind, regime, store, cap, qnorm))
                seen.add((store, rep[0], rep[1], min(rep[3], 2), cap, qnorm))
                n += 1
    for store in STORES:                                         # each mode in both kernel families, at every lane shape and over more than one chunk
        mine = [t for t in seen if t[0] == store]
        assert {t[1:3] for t in mine} == {(64, 4), (128, 2), (256, 1)}, (store, mine)
        assert any(t[3] >= 2 for t in mine), (store, mine)
        assert {t[4] for t in mine} == set(CAPS) and {t[5] for t in mine} == {0, 1}, (store, mine)
    worst.show('%d x %d, %d launches' % (nz, nx, n))


def test_every_launch_shape_is_reached(helm_lib):
    """what the reports of the cases above have to show between them: the three launch shapes, more than one chunk of 256 columns, fewer workgroups than
    tiles (the grid-stride loop over the banded tile order, whose 8 bands have holes when the tiles are no multiple of 8), fewer than 8 tiles"""
    reps = []
    for nz, nx in ((1, 1), (9, 70), (33, 65), (130, 3)):
        for ncol in (1, 65, 129, 300, 513):
            for cap in CAPS:
                C, x, q = rc.operands('random', nz, nx, ncol, 'random')
                reps.append(lean_resid(helm_lib, C, x, q, cap))
    assert {(r[0], r[1]) for r in reps} == {(64, 4), (128, 2), (256, 1)}
    assert any(r[3] == 2 for r in reps) and any(r[3] == 3 for r in reps)
    assert any(r[2] < r[4] and r[4] % 8 for r in reps) and any(r[2] < r[4] and r[1] == 1 for r in reps) and any(r[2] < r[4] and r[1] > 1 for r in reps)
    assert any(r[4] < 8 for r in reps) and any(r[4] > 8 and r[4] % 8 for r in reps)


def lean_resid(lib, C, x, q, cap):
    """a norms-only launch checked against the fp64 evaluation to 1e-12 (no extended-precision reference: the shapes are what this one is about)"""
    _, nz, nx = C.shape
    N, ncol = x.shape
    rcode, rep, rr, qq = rc.nm_stage(lib, rc.RESID, nz=nz, nx=nx, ncol=ncol, nblk_cap=cap, planes=np.ascontiguousarray(C).ravel(), Xin=x.ravel().copy(), ldin=ncol,
                                     Q=q.ravel().copy(), ldq=ncol, qnorm=1)
    assert rcode == 0
    check_report(rep, nz, nx, ncol, cap)
    _, rr64, qq64, _ = rc.resid_fp64(C, x, q)
    assert np.allclose(rr, rr64, rtol=1e-12, atol=0) and np.allclose(qq, qq64, rtol=1e-12, atol=0)
    return rep


# ---- 2. the column map ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [37, 100, 200, 300, 513])
def test_column_map(helm_lib, ncol):
    """qmap: a random choice of ncol distinct columns out of ldq > ncol, so the map reaches columns at or beyond ncol and the columns it leaves out (NaN on the
    way in) are nobody's; more than 256 columns: the later chunks take their part of the map"""
    worst, n = Worst(), 0
    for nz, nx in ((5, 33), (9, 70)):
        kind = rc.kind_for(nz, nx, n)
        for regime in ('random', 'cancel'):
            C, x, q = rc.operands(kind, nz, nx, ncol, regime)
            ref = rc.Ref(C, x, q)
            for store in (None, 'rout', 'inplace'):
                pad = n % 3
                ldq = ncol + PADS[(pad + 1) % 3]
                qmap = np.random.default_rng(n).permutation(ldq)[:ncol]
                if ldq - 1 not in qmap:
                    qmap[ncol // 2] = ldq - 1
                assert qmap.max() >= ncol and np.any(np.diff(qmap) < 0)
                ratios, _, _, _ = run_resid(helm_lib, C, x, q, ref, cap=CAPS[n % 3], store=store, qnorm=(n + 1) % 2, qmap=qmap, pad=pad)
                worst.add(ratios, (nz, nx, ncol, regime, store))
                n += 1
    worst.show('column map, %d columns' % ncol)


# ---- 3. the wavefield the launch writes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [1, 63, 128, 200, 300])
@pytest.mark.parametrize('oscale', rc.OSCALES, ids=['one', 'complex'])
def test_wavefield_output(helm_lib, ncol, oscale):
    """Uout = conj(oscale x) written by the launch that checks x (the node-major callers): with the norms alone, as the solver does it, and beside a stored r"""
    worst, n = Worst(), 0
    for nz, nx in ((3, 31), (9, 70)):
        C, x, q = rc.operands(rc.kind_for(nz, nx, n), nz, nx, ncol, ('random', 'cancel')[n % 2])
        ref = rc.Ref(C, x, q)
        for store in (None, 'rout'):
            ratios, _, _, _ = run_resid(helm_lib, C, x, q, ref, cap=CAPS[n % 3], store=store, qnorm=1, uout=True, oscale=oscale, pad=n)
            worst.add(ratios, (nz, nx, ncol, store))
            n += 1
    worst.show('Uout, %d columns, oscale %s' % (ncol, oscale))


# ---- 4. direct output: the launch reads u = conj(oscale x) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [129, 200, 256, 300, 513])
@pytest.mark.parametrize('oscale', rc.OSCALES, ids=['one', 'complex'])
def test_residual_from_the_wavefield_array(helm_lib, ncol, oscale):
    """xin_is_u: x = conj(u), q' = oscale q (oscale = 1: q itself), ||q'||^2 from the same launch as in true_residual_norms"""
    worst, n = Worst(), 0
    for nz, nx in ((5, 33), (9, 70)):
        for regime in ('random', 'cancel'):
            C, x, q = rc.operands(rc.kind_for(nz, nx, n), nz, nx, ncol, regime)
            u = np.conj(oscale * x)
            if regime == 'cancel' and oscale != 1:                    # q with oscale q = fl(A conj(u)) to rounding
                q = ho.stencil_apply(C, np.conj(u)) / oscale
            ref = rc.Ref(C, u, q, oscale=oscale, xin_is_u=True)
            assert ref.const == (24 if oscale == 1 else 28)
            for store in (None, 'rout'):
                ratios, _, _, _ = run_resid(helm_lib, C, u, q, ref, cap=CAPS[n % 3], store=store, qnorm=1, oscale=oscale, xin_is_u=1, pad=n)
                worst.add(ratios, (nz, nx, ncol, regime, store))
                n += 1
    worst.show('xin_is_u, %d columns, oscale %s' % (ncol, oscale))


@pytest.mark.parametrize('ncol', [1, 64, 128])
def test_narrow_batches_refuse_the_wavefield_array(helm_lib, ncol):
    """nd_resid_nm: direct output needs the full-width kernel -- HELM_ERR_STATE, nothing written"""
    C, x, q = rc.operands('random', 5, 33, ncol, 'random')
    for oscale in rc.OSCALES:
        run_resid(helm_lib, C, np.conj(oscale * x), q, None, store='rout', uout=True, oscale=oscale, xin_is_u=1, expect=rc.HELM_ERR_STATE)


# ---- 5. sparse right-hand sides ----------------------------------------------------------------------------------------------------------------------------------
def cell_mask(rng, nz, nx):
    """a byte per cell, different from cell to cell and from block to block of 64 columns (the bits above the four blocks random as well), with fixed patterns
    on the first two and the last column of the 32-cell segments"""
    m = rng.integers(0, 256, size=(nz, nx)).astype(np.uint8)
    for x0 in range(0, nx, 32):
        for dx, pat in ((0, 0b0101), (1, 0b1010), (31, 0b0110)):
            if x0 + dx < nx:
                m[::2, x0 + dx] = pat
                m[1::2, x0 + dx] = pat ^ 0b1111
    m[nz // 2, nx // 2], m[0, nx - 1] = 0, 0xF
    return m


@pytest.mark.parametrize('ncol', [64, 100, 129, 200, 256, 300])
def test_right_hand_side_mask(helm_lib, ncol):
    """qmask: Q holds NaN wherever its (cell, block of 64 columns) bit is 0 and the reference takes 0 there -- a mask read one column or one block off poisons
    the result or drops a nonzero q.  Beyond the first 256 columns the launch has no mask and reads all of q.  The narrow kernel takes no mask at all (the
    launcher hands it none): there Q holds the zeros the mask promises."""
    worst, n = Worst(), 0
    for nz, nx in ((5, 33), (9, 70), (33, 65)):
        rng = np.random.default_rng(nz + ncol)
        mask = cell_mask(rng, nz, nx)
        j = np.arange(ncol)
        keep = ((mask.reshape(-1, 1) >> np.minimum(j // 64, 7)[None, :]) & 1).astype(bool) | (j >= 256)[None, :]
        assert keep.any() and not keep.all()
        for regime in ('random', 'cancel'):
            C, x, q = rc.operands(rc.kind_for(nz, nx, n), nz, nx, ncol, regime)
            ref = rc.Ref(C, x, q, qkeep=keep)
            q_in = np.where(keep, q, NAN if ncol > 128 else 0)
            for store in (None, 'rout'):
                ratios, rep, _, _ = run_resid(helm_lib, C, x, q, ref, cap=CAPS[n % 3], store=store, qnorm=1, qmask=mask.ravel(), q_in=q_in, pad=n)
                assert (rep[1] == 1) == (ncol > 128)
                worst.add(ratios, (nz, nx, ncol, regime, store))
                n += 1
    worst.show('qmask, %d columns' % ncol)


# ---- 6. the right-hand-side preparation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 31, 32, 33, 1000])
def test_prep_transpose_norm(helm_lib, N):
    """Qt[i][r] = premul rhs[r][row_off + i] - sub[r][i] and ||.||^2 of what was stored: the window inside rows of rhs_ld with NaN outside it"""
    rng = np.random.default_rng(N)
    tiles = (N + 31) // 32
    worst, n = Worst(), 0
    for nrhs in (1, 31, 32, 33, 70):
        for row_off in (0, 5):
            for premul in (1 + 0j, 0.5 - 2j):
                for with_sub in (False, True):
                    cap = (1, 1024, tiles + 5)[n % 3]
                    rhs_ld = row_off + N + PADS[n % 3]
                    win = crand(rng, nrhs, N) * np.ldexp(1.0, rng.integers(-6, 7, size=(nrhs, 1)))
                    rhs = np.full((nrhs + 1, rhs_ld), NAN)
                    rhs[:nrhs, row_off:row_off + N] = win
                    sub = crand(rng, nrhs, N) if with_sub else None
                    subb = np.vstack([sub, np.full((1, N), NAN)]) if with_sub else None
                    Qt = np.full((N + 1, nrhs), SENT)
                    rcode, rep, _, qq = rc.nm_stage(helm_lib, rc.PREP, N=N, ncol=nrhs, nblk_cap=cap, Xin=rhs.ravel(), rhs_ld=rhs_ld, row_off=row_off, oscale=premul,
                                                    Q=None if subb is None else subb.ravel(), Rout=Qt.ravel())
                    assert rcode == 0
                    assert rep[2] == max(1, min(tiles, cap, 1024)) and rep[4] == tiles, rep
                    assert np.all(Qt[N] == SENT) and not np.any(Qt[:N] == SENT)
                    assert subb is None or np.array_equal(bits(subb[:nrhs]), bits(sub)) and np.all(np.isnan(subb[nrhs])), 'PREP wrote to sub'
                    s = (np.abs(Qt[:N].astype(rc.CLD)) ** 2).sum(axis=0)
                    ratios = dict(Qt=rc.ratio_prep(Qt[:N], win, premul, sub), qq=rc.ratio(np.abs(qq.astype(rc.LD) - s), (2 * N + 8) * U * s))
                    worst.add(ratios, (N, nrhs, row_off, premul, with_sub, cap))
                    n += 1
    worst.show('PREP, N %d, %d launches' % (N, n))


# ---- 7. the pass-throughs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,n', [(77, 20), (1, 4), (1031, 8)])
def test_pack_and_scatter_add(helm_lib, N, n):
    """k_pack_cols and k_scatter_add_cols, the minority pass: k = 1, 3 and n / 2 - 1 columns in no order, N k no multiple of 256; packing moves bits, the
    scatter adds with one rounding per component (the fp64 sum), every other column and the padding stay"""
    rng = np.random.default_rng(N)
    for k in sorted({1, 3, n // 2 - 1}):
        assert (N * k) % 256
        ld = n + 3
        cols = rng.permutation(n)[:k]
        if k > 1:
            cols[:2] = sorted(cols[:2])[::-1]
        Qt = padded(crand(rng, N, n), ld, NAN)
        Rp = np.full(N * k + 7, SENT)
        rcode = rc.nm_stage(helm_lib, rc.PACK, N=N, ncol=k, Xin=Qt.ravel(), ldin=ld, qmap=cols.astype(np.int32), Rout=Rp)[0]
        assert rcode == 0
        assert rc.same_bits(Rp[:N * k].reshape(N, k), Qt[:N, cols]) and np.all(Rp[N * k:] == SENT), 'PACK k %d' % k
        Xt = padded(crand(rng, N, n), ld, SENT)
        X0 = Xt.copy()
        Dp = np.concatenate([(crand(rng, N, k) * 1e-3).ravel(), np.full(5, NAN)])
        rcode = rc.nm_stage(helm_lib, rc.SCATTER_ADD, N=N, ncol=k, Xin=Dp, Q=Xt.ravel(), ldq=ld, qmap=cols.astype(np.int32))[0]
        assert rcode == 0
        want = X0.copy()
        want[:N, cols] = X0[:N, cols] + Dp[:N * k].reshape(N, k)
        assert np.array_equal(bits(Xt), bits(want)), 'SCATTER_ADD k %d' % k
    print('PACK / SCATTER_ADD %d x %d: bit for bit' % (N, n))


def test_recover_x(helm_lib):
    """Xt = conj(U) / oscale: the same bits when oscale = 1; otherwise the reciprocal (two products, a sum, two quotients: 3 u) and one complex multiply
    (sqrt(2) gamma_2 < 3 u): within 8 u |U| / |oscale|"""
    rng = np.random.default_rng(8)
    for N, ncol in ((1, 1), (77, 5), (1031, 70)):
        Ub = np.concatenate([crand(rng, N * ncol), np.full(3, NAN)])
        for oscale in rc.OSCALES:
            X = np.full(N * ncol + 3, SENT)
            assert rc.nm_stage(helm_lib, rc.RECOVER_X, N=N, ncol=ncol, Xin=Ub, Rout=X, oscale=oscale)[0] == 0
            assert np.all(X[N * ncol:] == SENT)
            u = Ub[:N * ncol]
            if oscale == 1:
                assert rc.same_bits(X[:N * ncol], np.conj(u))
            else:
                w = rc.ratio(np.abs(X[:N * ncol].astype(rc.CLD) - np.conj(u.astype(rc.CLD)) / rc.CLD(oscale)), 8 * U * np.abs(u) / abs(oscale))
                print('RECOVER_X %d x %d: worst |out - ref| / bound = %.4f' % (N, ncol, w))
                assert w <= 1.0


@pytest.mark.parametrize('N,ncol', [(1, 1), (31, 33), (33, 33), (1000, 7), (7, 1000), (1031, 70)])
def test_transposes(helm_lib, N, ncol):
    """nd_transpose_out with and without conj, nd_transpose on both sides of rows > cols: bits moved, nothing else written"""
    rng = np.random.default_rng(N + ncol)
    Xt = np.concatenate([crand(rng, N * ncol), np.full(33, NAN)])
    X2 = Xt[:N * ncol].reshape(N, ncol)
    for stage, conj in ((rc.TRANSPOSE_OUT, 0), (rc.TRANSPOSE_OUT, 1), (rc.TRANSPOSE, 0)):
        out = np.full(N * ncol + 33, SENT)
        assert rc.nm_stage(helm_lib, stage, N=N, ncol=ncol, Xin=Xt, Rout=out, conj=conj)[0] == 0
        assert rc.same_bits(out[:N * ncol].reshape(ncol, N), np.conj(X2.T) if conj else X2.T) and np.all(out[N * ncol:] == SENT), (stage, conj)


# ---- 8. the minority pass, in the order of direct_batch_nm --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncol', [40, 200])
def test_minority_pass_composed(helm_lib, ncol):
    """RESID with store writes Rt, PACK packs the columns above the tolerance, the correction comes from the oracle's LU on the host, SCATTER_ADD adds it back,
    RESID norms again: the refined columns drop below 1e-12, every other column has the bits of the first evaluation"""
    nz, nx = 9, 70
    N = nz * nx
    C = rc.planes_of('mz', nz, nx)
    rng = np.random.default_rng(ncol)
    q = crand(rng, N, ncol)
    lu = ho.DirectOperator(C).factor()
    x = lu.solve(q)
    bad = rng.permutation(ncol)[:ncol // 2 - 1]
    x[:, bad] *= 1 + 1e-6 * rng.standard_normal((N, bad.size))
    ld = ncol + 3
    planes = np.ascontiguousarray(C).ravel()

    def norms(Xb):
        Qb = padded(q, ld, NAN)
        rcode, _, rr, qq = rc.nm_stage(helm_lib, rc.RESID, nz=nz, nx=nx, ncol=ncol, planes=planes, Xin=Xb.ravel(), ldin=ld, Q=Qb.ravel(), ldq=ld, qnorm=1)
        assert rcode == 0
        return rr, qq
    Xb = padded(x, ld, NAN)
    rr0, qq0 = norms(Xb)
    rel0 = np.sqrt(rr0 / qq0)
    assert np.all(rel0[bad] > 1e-9) and np.all(np.delete(rel0, bad) < 1e-12), rel0
    Qb, Rt = padded(q, ld, NAN), np.full((N + 1, ld), SENT)
    assert rc.nm_stage(helm_lib, rc.RESID, nz=nz, nx=nx, ncol=ncol, planes=planes, Xin=Xb.ravel(), ldin=ld, Q=Qb.ravel(), ldq=ld, store=1, Rout=Rt.ravel())[0] == 0
    k = bad.size
    Rp = np.full(N * k, SENT)
    assert rc.nm_stage(helm_lib, rc.PACK, N=N, ncol=k, Xin=Rt.ravel(), ldin=ld, qmap=bad.astype(np.int32), Rout=Rp)[0] == 0
    Dp = np.ascontiguousarray(lu.solve(Rp.reshape(N, k)))
    X1 = Xb.copy()
    assert rc.nm_stage(helm_lib, rc.SCATTER_ADD, N=N, ncol=k, Xin=Dp.ravel(), Q=X1.ravel(), ldq=ld, qmap=bad.astype(np.int32))[0] == 0
    rr1, qq1 = norms(X1)
    rel1 = np.sqrt(rr1 / qq1)
    others = np.setdiff1d(np.arange(ncol), bad)
    print('minority pass, %d of %d columns: relres %.2e -> %.2e' % (k, ncol, rel0[bad].max(), rel1[bad].max()))
    assert np.all(rel1[bad] < 1e-12), rel1[bad].max()
    assert np.array_equal(rr1[others].view(np.uint64), rr0[others].view(np.uint64)) and np.array_equal(qq1.view(np.uint64), qq0.view(np.uint64))
    assert np.array_equal(bits(X1[:, others]), bits(Xb[:, others]))
