"""GPU: every instantiation and addressing mode of the tile kernel k_zgemm3 (zephyr_amd/csrc/nd_gemm.hip, nd_gemm_body.hpp) against the same product in
numpy.clongdouble, through the test hook helm_debug_zgemm_ex.

Bound, for every element (u = 2^-53):

    |out - ref|_ij <= 4 (K + 4) u ( |alpha| (|A| |B|)_ij + |beta| |C_ij| )

which every summation order of an fp64 complex dot product satisfies, with or without FMA (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and
3.6: gamma_K for the sum, sqrt(2) gamma_2 per complex multiply; the factor 4 covers both and the final alpha / beta step).  Outputs that go through
conj(oscale x) (cj_out, Cox2) carry one more complex multiply: |oscale| times the bound with K + 5 in the place of K + 4.  An element whose bound is zero
has to be exact.  Every test prints the launch that ran (tile / K slab / XR / split) and the worst ratio |out - ref| / bound it saw.

Every dense operand lies in a buffer whose padding (between rows when ld > width, between batch items, one row past the end) holds NaN for A and B and a
sentinel for C: a read outside an operand poisons the result, and the sentinel has to come back bit for bit.  An operand that is a sub-block of a larger
matrix is exactly that: a leading dimension larger than the width, the neighbours being the larger matrix' other columns.  (The hook's buffers begin at an
operand's first element, so what lies before it in a larger matrix is not represented; what lies beside and behind it is.)

Not covered here: the forward-gather and Schur-gather modes (IDX 2 and 4), which need the plan's node records and the children's arenas, and the kernels
k_leaf_bwd_idle and k_sep_bwd_small; they are reached from inside a solve only (tests/test_gpu_direct.py)."""
import numpy as np
import pytest

from tests import zgemm_shapes as zs

pytestmark = pytest.mark.gpu
SENT = complex(-1.2345e300, 6.789e-300)
PADS = ((0, 0, 0), (1, 3, 61), (3, 61, 1), (61, 1, 3))


@pytest.fixture(autouse=True)
def _x87():
    if not zs.have_x87():
        pytest.skip('numpy.longdouble is not the 80-bit x87 format on this host: no extended-precision reference')


def forcing(name):
    tile, slab, xr = zs.INSTANTIATIONS[name]
    return {} if xr else dict(force_tile=tile, force_slab=slab)


def dims(name):
    """M and N values of an instantiation: tile size - 1, tile size, tile size + 1, 1, two-and-a-bit tiles (tile 8: at most 16 columns, as in production;
    XR: 49 rows and at least 64 columns, anything else is another instantiation)"""
    tile, _, xr = zs.INSTANTIATIONS[name]
    if xr:
        return (49,), (64, 65, 127, 128, 129, 137)
    tm, tn = zs.TILES[tile]
    Ms = (tm - 1, tm, tm + 1, 1, 2 * tm + max(5, tm // 8))
    Ns = (15, 16, 1, 7, 9) if tile == 8 else (tn - 1, tn, tn + 1, 1, 2 * tn + 9)
    return Ms, Ns


class Dense(object):
    """one dense problem: operands in padded buffers, the extended-precision product, and the check of a run"""

    def __init__(self, rng, M, N, K, batch, pads=(0, 0, 0), gaps=(0, 0, 0), sa0=False, sb0=False, mixed=False, brows=None):
        self.M, self.N, self.K, self.batch = M, N, K, batch
        brows = brows or K
        self.lda, self.ldb, self.ldc = K + pads[0], N + pads[1], N + pads[2]
        ia, ib, self.ic = M * self.lda + gaps[0], brows * self.ldb + gaps[1], M * self.ldc + gaps[2]
        self.sa, self.sb, self.sc = (0 if sa0 else ia), (0 if sb0 else ib), self.ic
        na, nb = (1 if sa0 else batch), (1 if sb0 else batch)
        A, B = zs.crand(rng, na, M, K), zs.crand(rng, nb, brows, N)
        if mixed:
            A = zs.mixed_rows(rng, A)
        self.C0 = zs.crand(rng, batch, M, N)
        self.Abuf = np.full(na * ia + self.lda, np.nan + 1j * np.nan)
        self.Bbuf = np.full(nb * ib + self.ldb, np.nan + 1j * np.nan)
        self.view(self.Abuf, na, M, K, self.lda, ia)[...] = A
        self.view(self.Bbuf, nb, brows, N, self.ldb, ib)[...] = B
        ld = np.clongdouble                                      # (a shared operand is converted once and broadcast by matmul)
        self.P = np.broadcast_to(np.matmul(A.astype(ld), B[:, :K].astype(ld)), (batch, M, N))
        self.SP = np.broadcast_to(np.matmul(np.abs(A), np.abs(B[:, :K])), (batch, M, N))

    @staticmethod
    def view(buf, batch, rows, cols, ld, stride):
        it = buf.itemsize
        return np.lib.stride_tricks.as_strided(buf, shape=(batch, rows, cols), strides=(stride * it, ld * it, it))

    def run(self, lib, alpha, beta, zr=(0, 0), zc=(0, 0), sk=(0, 0), **opt):
        M, N, K, batch = self.M, self.N, self.K, self.batch
        Cbuf = np.full(batch * self.ic + self.ldc, SENT)
        cv = self.view(Cbuf, batch, M, N, self.ldc, self.ic)
        cv[...] = self.C0 if beta != 0 else np.nan           # beta == 0 must not read C
        Cin = self.C0.copy()
        for (lo, hi), ax in ((zr, 1), (zc, 2)):                # masked rows / columns: taken as zero, and must not be read
            sl = [slice(None)] * 3
            sl[ax] = slice(lo, hi)
            cv[tuple(sl)] = np.nan
            Cin[tuple(sl)] = 0
        cv[:, sk[0]:sk[1], sk[0]:sk[1]] = SENT                  # neither read nor written
        before = Cbuf.copy()
        rc, rep = zs.zgemm_ex(lib, M, N, K, batch, self.Abuf, self.lda, self.sa, self.Bbuf, self.ldb, self.sb, Cbuf, self.ldc, self.sc, alpha, beta,
                              zr=zr, zc=zc, sk=sk, **opt)
        assert rc == 0, rc
        out = cv.copy()
        ref = np.clongdouble(alpha) * self.P
        S = abs(alpha) * self.SP
        if beta != 0:
            ref = ref + np.clongdouble(beta) * Cin.astype(np.clongdouble)
            S = S + abs(beta) * np.abs(Cin)
        # everything but the interior, and the sk block inside it, comes back bit for bit
        cv[...] = 0
        self.view(before, batch, M, N, self.ldc, self.ic)[...] = 0
        assert np.array_equal(Cbuf.view(np.uint64), before.view(np.uint64)), 'the launch wrote outside C'
        if sk[1] > sk[0]:
            blk = out[:, sk[0]:sk[1], sk[0]:sk[1]]
            assert np.array_equal(blk.copy().view(np.uint64), np.full_like(blk, SENT).view(np.uint64)), 'the sk block was written'
            out[:, sk[0]:sk[1], sk[0]:sk[1]] = ref[:, sk[0]:sk[1], sk[0]:sk[1]].astype(np.complex128)
            S = S.copy()
            S[:, sk[0]:sk[1], sk[0]:sk[1]] = np.inf
        return zs.worst_ratio(out, ref, S, K), rep


def check(worst, what):
    print('%s: worst |out - ref| / bound = %.4f' % (what, worst))
    assert worst <= 1.0, what


def ran(name, rep):
    assert zs.instantiation_of(rep) == name and rep[3] == 0, 'meant %s, ran %s' % (name, rep)
    return 'tile %s slab %d XR %d split %d' % ((rep[0] if not rep[2] else '49x64'), rep[1], rep[2], rep[3])


# ---- 1. every instantiation, dense --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(zs.INSTANTIATIONS))
def test_every_instantiation_on_tile_borders_and_every_k_remainder(helm_lib, name):
    """M, N around the tile borders x every K of K_LIST x the three (alpha, beta) pairs, one matrix; the paddings of the leading dimensions cycle with the
    shape, rows of A of mixed magnitude on every other shape."""
    rng = np.random.default_rng(sorted(zs.INSTANTIATIONS).index(name))
    Ms, Ns = dims(name)
    worst, n, desc = 0.0, 0, ''
    for M in Ms:
        for N in Ns:
            for K in zs.K_LIST:
                p = Dense(rng, M, N, K, 1, pads=PADS[n % 4], mixed=bool(n & 1))
                n += 1
                for alpha, beta in zs.ALPHA_BETA:
                    w, rep = p.run(helm_lib, alpha, beta, **forcing(name))
                    desc = ran(name, rep)
                    assert w <= 1.0, (name, M, N, K, alpha, beta, w)
                    worst = max(worst, w)
    check(worst, '%s [%s], %d shapes' % (name, desc, n))


@pytest.mark.parametrize('name', sorted(zs.INSTANTIATIONS))
def test_every_instantiation_batched_under_every_xcd_map(helm_lib, name):
    """batch 3 and 19 (a tail of three beside two blocks of eight for the regrouping of the workgroup ids) for nd_xcd_map 0, 1, 2: one row tile and several,
    with and without nontemporal stores"""
    rng = np.random.default_rng(100 + sorted(zs.INSTANTIATIONS).index(name))
    Ms, Ns = dims(name)
    worst, desc = 0.0, ''
    for M, N in ((Ms[-1], Ns[-1]), (Ms[0], Ns[-1]), (Ms[-1], Ns[2])):
        for batch in (3, 19):
            p = Dense(rng, M, N, 17, batch, pads=(1, 3, 61), mixed=True)
            for i, xcd in enumerate((0, 1, 2)):
                alpha, beta = zs.ALPHA_BETA[(i + batch) % 3]
                w, rep = p.run(helm_lib, alpha, beta, xcd_map=xcd, ntc=i & 1, **forcing(name))
                desc = ran(name, rep)
                assert w <= 1.0, (name, M, N, batch, xcd, w)
                worst = max(worst, w)
    check(worst, '%s [%s], batched' % (name, desc))


@pytest.mark.parametrize('name', sorted(zs.NATURAL))
def test_natural_choice_runs_the_instantiation_it_is_listed_for(helm_lib, name):
    M, N, K, batch = zs.NATURAL[name]
    p = Dense(np.random.default_rng(M + N), M, N, K, batch, mixed=True)
    worst = 0.0
    for alpha, beta in zs.ALPHA_BETA:
        w, rep = p.run(helm_lib, alpha, beta)
        desc = ran(name, rep)
        worst = max(worst, w)
    check(worst, '%s natural %s [%s]' % (name, zs.NATURAL[name], desc))


# ---- 2. leading dimensions and strides --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tile0-slab8', 'tile1-slab8', 'tile3-slab8', 'tile6-slab16', 'tile7-slab8', 'tile8-slab8', 'xr'])
@pytest.mark.parametrize('sa0,sb0', [(False, False), (True, False), (False, True), (True, True)], ids=['own', 'sa0', 'sb0', 'sa0-sb0'])
def test_leading_dimensions_strides_and_shared_operands(helm_lib, name, sa0, sb0):
    """lda > K, ldb > N, ldc > N by 1, 3 and 61 in every arrangement, batch strides larger than the matrices, A and / or B shared by the batch (stride 0)"""
    rng = np.random.default_rng(7)
    Ms, Ns = dims(name)
    worst = 0.0
    for pads in PADS[1:]:
        for M, N in ((Ms[min(2, len(Ms) - 1)], Ns[-1]), (Ms[-1], Ns[0])):
            p = Dense(rng, M, N, 21, 5, pads=pads, gaps=(5, 130, 77), sa0=sa0, sb0=sb0, mixed=True)
            for alpha, beta in zs.ALPHA_BETA[::2]:
                w, rep = p.run(helm_lib, alpha, beta, **forcing(name))
                desc = ran(name, rep)
                assert w <= 1.0, (name, M, N, pads, w)
                worst = max(worst, w)
    check(worst, '%s [%s], paddings and strides' % (name, desc))


# ---- 3. masks and in-place -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tile0-slab8', 'tile1-slab8', 'tile2-slab8', 'tile3-slab8', 'tile4-slab8', 'tile5-slab8', 'tile6-slab8', 'tile6-slab16',
                                  'tile7-slab8', 'tile7-slab16'])
def test_masks(helm_lib, name):
    """zr / zc ranges that begin and end inside a block of 16 rows and across tile borders, beta = 1, NaN in C where it is masked; the sk block keeps its
    sentinel"""
    rng = np.random.default_rng(11)
    tm, tn = zs.TILES[zs.INSTANTIATIONS[name][0]]
    M, N = 2 * tm + 7, 2 * tn + 9
    p = Dense(rng, M, N, 13, 3, pads=(0, 3, 1), mixed=True)
    worst = 0.0
    for zr, zc, sk in (((3, 11), (0, 0), (0, 0)), ((0, 0), (5, 14), (0, 0)), ((tm - 3, tm + 5), (tn - 2, tn + 19), (0, 0)), ((0, M), (0, 0), (0, 0)),
                       ((0, 0), (0, N), (0, 0)), ((0, 0), (0, 0), (5, 14)), ((2, tm + 1), (tn, N), (tm - 5, tm + 6)), ((M - 1, M), (N - 1, N), (0, min(M, N)))):
        for alpha, beta in ((-1 + 0j, 1 + 0j), (0.3 - 0.2j, 0.5 + 0.1j)):
            w, rep = p.run(helm_lib, alpha, beta, zr=zr, zc=zc, sk=sk, **forcing(name))
            desc = ran(name, rep)
            assert w <= 1.0, (name, zr, zc, sk, w)
            worst = max(worst, w)
    check(worst, '%s [%s], masks' % (name, desc))


@pytest.mark.parametrize('M,N,K,tile', [(16, 200, 16, 7), (9, 70, 9, 7), (1, 1, 1, 7), (40, 32, 40, 3), (64, 17, 64, 3), (17, 7, 30, 3), (64, 300, 64, 0),
                                        (33, 33, 33, 0), (50, 129, 64, 0), (64, 64, 17, 0)])
def test_in_place_one_row_tile_per_matrix(helm_lib, M, N, K, tile):
    """tm64: C over B (M <= 16: 16 x 64 tiles, N <= 32: 64 x 32, else 64 x 64) against the out-of-place reference; the rows of B below C stay as they were"""
    rng = np.random.default_rng(M * 1000 + N)
    batch, pad = 21, 3
    rows = max(M, K)
    p = Dense(rng, M, N, K, batch, pads=(1, pad, pad), gaps=(0, 11, 11), brows=rows)
    worst = 0.0
    for alpha in (1 + 0j, 0.3 - 0.2j):
        Bbuf = p.Bbuf.copy()
        before = Bbuf.copy()
        rc, rep = zs.zgemm_ex(helm_lib, M, N, K, batch, p.Abuf, p.lda, p.sa, Bbuf, p.ldb, p.sb, None, p.ldb, p.sb, alpha, 0j, tm64=1, c_is_b=1)
        assert rc == 0 and rep[:4] == (tile, 8, 0, 0), rep
        ib = rows * p.ldb + 11
        out = p.view(Bbuf, batch, M, N, p.ldb, ib).copy()
        w = zs.worst_ratio(out, np.clongdouble(alpha) * p.P, abs(alpha) * p.SP, K)
        p.view(Bbuf, batch, M, N, p.ldb, ib)[...] = 0
        p.view(before, batch, M, N, p.ldb, ib)[...] = 0
        assert np.array_equal(Bbuf.view(np.uint64), before.view(np.uint64)), 'the launch wrote outside C'
        assert w <= 1.0, (M, N, K, alpha, w)
        worst = max(worst, w)
    check(worst, 'in place %d x %d x %d [tile %d slab %d]' % (M, N, K, rep[0], rep[1]))


# ---- 4. row-table mode ------------------------------------------------------------------------------------------------------------------------------------
class Table(object):
    """one row-table problem: A dense, the rows of B / of the C that is read / of the C that is written looked up in node-major arenas"""

    def __init__(self, rng, M, N, K, batch, k2=0, ldx_pad=3, neg=0.15, arena_rows=None, mixed=True):
        self.M, self.N, self.K, self.batch, self.k2 = M, N, K, batch, k2
        self.ldx = N + ldx_pad
        self.rows = R = arena_rows or max(batch * M + 40, 300)
        self.stride = K + 2 * M + 5
        self.offB, self.offCi, self.offCo = 2, K + 3, K + M + 4
        A = zs.crand(rng, batch, M, K)
        self.A = zs.mixed_rows(rng, A) if mixed else A
        self.Abuf = np.ascontiguousarray(self.A).ravel()
        tab = np.full((batch, self.stride), -7, np.int32)            # (entries no operand owns: never looked up)
        tB = rng.integers(0, R, size=(batch, K))
        tB[:, 1::5] = tB[:, 0:1]                                      # repeats
        tB[rng.random((batch, K)) < neg] = -1                         # zero rows of B
        tCi = rng.integers(0, R, size=(batch, M))
        tCi[rng.random((batch, M)) < neg] = -1                        # no C read
        tCo = rng.permutation(R)[:batch * M].reshape(batch, M)        # every stored row has one writer
        tCo[rng.random((batch, M)) < neg] = -1                        # rows that are not stored
        tab[:, self.offB:self.offB + K], tab[:, self.offCi:self.offCi + M], tab[:, self.offCo:self.offCo + M] = tB, tCi, tCo
        self.tab, self.tB, self.tCi, self.tCo = tab.ravel(), tB, tCi, tCo

        def arena(fill=None):
            a = np.full((R, self.ldx), np.nan + 1j * np.nan) if fill is None else np.full((R, self.ldx), fill)
            if fill is None:
                a[:, :N] = zs.crand(rng, R, N)
            return a
        self.Bx, self.Bx2, self.Cix = arena(), arena(), arena()
        self.new_out = lambda: arena(SENT)

    def gathered(self):
        Bz = np.where((np.arange(self.K) < self.k2)[None, :, None], self.Bx2[:, :self.N][self.tB], self.Bx[:, :self.N][self.tB])
        Bz[self.tB < 0] = 0
        Cz = self.Cix[:, :self.N][self.tCi]
        Cz[self.tCi < 0] = 0
        return Bz, Cz

    def run(self, lib, alpha, beta, cj_out=0, oscale=1 + 0j, second=False, tabCi=True, **opt):
        M, N, K, batch = self.M, self.N, self.K, self.batch
        Cox, Cox2 = self.new_out().ravel(), (self.new_out().ravel() if second else None)
        rc, rep = zs.zgemm_ex(lib, M, N, K, batch, self.Abuf, K, M * K, None, 0, 0, None, 0, 0, alpha, beta,
                              tabB=self.tab, tabCi=self.tab if tabCi else None, tabCo=self.tab, tab_stride=self.stride, offB=self.offB, offCi=self.offCi,
                              offCo=self.offCo, ldx=self.ldx, arena_rows=self.rows, Bx=self.Bx.ravel(), Bx2=self.Bx2.ravel() if self.k2 else None,
                              Cix=self.Cix.ravel() if tabCi else None, Cox=Cox, Cox2=Cox2, k2=self.k2, cj_out=cj_out, oscale=oscale, **opt)
        assert rc == 0, rc
        Bz, Cz = self.gathered()
        ref, S = zs.reference(self.A, Bz, Cz, alpha, beta)
        stored = self.tCo >= 0
        rows = self.tCo[stored]
        worst = 0.0
        for arr, conj in ((Cox, cj_out), (Cox2, 2 if cj_out else 1)):
            if arr is None:
                continue
            arr = arr.reshape(self.rows, self.ldx)
            r, s, extra = ref[stored], S[stored], 0
            for _ in range(conj):                                        # conj(oscale x), once or (Cox2 of a cj_out launch) twice
                r, s, extra = np.conj(np.clongdouble(oscale) * r), abs(oscale) * s, extra + 1
            worst = max(worst, zs.worst_ratio(arr[rows, :N], r, s, K, extra))
            keep = arr.copy()
            keep[rows, :N] = SENT                                        # every other row, and the padding of every row, kept its sentinel
            assert np.array_equal(keep.view(np.uint64), np.full_like(keep, SENT).view(np.uint64)), 'a row without an output entry, or padding, was written'
        return worst, rep


TABLE_CASES = [(name, K, k2) for name in ('tile0-slab8', 'tile1-slab8', 'tile2-slab8', 'tile3-slab8', 'tile4-slab8', 'tile5-slab8', 'tile6-slab8', 'tile6-slab16',
                                          'tile7-slab8', 'tile7-slab16', 'xr') for K, k2 in ((37, 0), (81, 48), (512, 17))]


@pytest.mark.parametrize('name,K,k2', TABLE_CASES, ids=['%s-K%d-k2_%d' % c for c in TABLE_CASES])
def test_row_tables(helm_lib, name, K, k2):
    """tabB / tabCi random with repeats and negative entries, tabCo a permutation with negative entries; k2 = 0, on a slab border (48) and inside a slab (17) with
    Bx2 != Bx; K up to GB_KIDX; plain output, cj_out with a complex oscale, and the second copy Cox2"""
    rng = np.random.default_rng(K + k2)
    Ms, Ns = dims(name)
    M, N = Ms[-1], (Ns[-1] if K < 512 else Ns[2])
    batch = 19 if K < 512 else 3
    t = Table(rng, M, N, K, batch, k2=k2)
    worst = 0.0
    osc = 0.6 - 1.3j
    for alpha, beta, kw in ((1 + 0j, 0j, {}), (-1 + 0j, 1 + 0j, {}), (0.3 - 0.2j, 0.5 + 0.1j, dict(cj_out=1, oscale=osc)),
                            (-1 + 0j, 1 + 0j, dict(second=True, oscale=osc)), (1 + 0j, 0j, dict(second=True, oscale=osc, tabCi=False, ntc=1, xcd_map=1))):
        w, rep = t.run(helm_lib, alpha, beta, **dict(kw, **forcing(name)))
        desc = ran(name, rep)
        assert w <= 1.0, (name, K, k2, alpha, beta, sorted(kw), w)
        worst = max(worst, w)
    check(worst, '%s [%s], row tables K %d k2 %d' % (name, desc, K, k2))


@pytest.mark.parametrize('name', ['tile0-slab8', 'tile1-slab8', 'tile2-slab8', 'tile3-slab8', 'tile4-slab8', 'tile5-slab8', 'tile6-slab8', 'tile6-slab16',
                                  'tile7-slab8', 'tile7-slab16', 'tile8-slab8', 'xr'])
@pytest.mark.parametrize('k2', [0, 11])
def test_sparse_right_hand_side_flags(helm_lib, name, k2):
    """act without hint: the flags that come back say, per item and block of 64 columns, whether the gathered B rows hold a nonzero there (-0.0 is zero);
    on tiles of at least 64 columns the output rows of a block whose flag stays 0 keep their sentinel, narrower tiles store zeros"""
    rng = np.random.default_rng(5 + k2)
    Ms, Ns = dims(name)
    tile = zs.INSTANTIATIONS[name][0]
    M, N = Ms[min(2, len(Ms) - 1)], (16 if tile == 8 else 200)
    K, batch = 29, 23
    nct = (N + 63) // 64
    t = Table(rng, M, N, K, batch, k2=k2, arena_rows=batch * max(M, K) + 10, neg=0.1)
    # every item has rows of its own in the arenas: its blocks of 64 columns are made zero, or zero but for ONE entry, independently of the other items
    own = np.arange(batch)[:, None] * K + rng.permuted(np.tile(np.arange(K), (batch, 1)), axis=1)
    t.tB = np.where(t.tB < 0, -1, own)
    t.tab.reshape(batch, t.stride)[:, t.offB:t.offB + K] = t.tB
    want = np.zeros((batch, nct), np.int32)
    for z in range(batch):
        for j in range(nct):
            kind = rng.integers(0, 3)                           # 0: all zero (with -0.0 among them), 1: one nonzero entry, 2: dense
            c0, c1 = 64 * j, min(N, 64 * j + 64)
            if kind == 2:
                want[z, j] = 1 if (t.tB[z] >= 0).any() else 0
                continue
            for k in range(K):
                if t.tB[z, k] >= 0:
                    zero = np.zeros(c1 - c0, complex)
                    zero.real, zero.imag = np.where(rng.random(c1 - c0) < 0.5, 0.0, -0.0), np.where(rng.random(c1 - c0) < 0.5, 0.0, -0.0)
                    (t.Bx2 if k < k2 else t.Bx)[t.tB[z, k], c0:c1] = zero
            live = np.flatnonzero(t.tB[z] >= 0)
            if kind == 1 and live.size:
                k = rng.choice(live)
                (t.Bx2 if k < k2 else t.Bx)[t.tB[z, k], rng.integers(c0, c1)] = [1e-300, 1e-300j, -2.5 + 1j][rng.integers(0, 3)]
                want[z, j] = 1
    act = np.full(batch * nct, 77, np.int32)
    Cox = t.new_out().ravel()
    rc, rep = zs.zgemm_ex(helm_lib, M, N, K, batch, t.Abuf, K, M * K, None, 0, 0, None, 0, 0, 1 + 0j, 0j, tabB=t.tab, tabCo=t.tab, tab_stride=t.stride, offB=t.offB,
                          offCo=t.offCo, ldx=t.ldx, arena_rows=t.rows, Bx=t.Bx.ravel(), Bx2=t.Bx2.ravel() if k2 else None, Cox=Cox, k2=k2, act=act, **forcing(name))
    assert rc == 0
    desc = ran(name, rep)
    assert np.array_equal(act.reshape(batch, nct), want), 'flags differ from "a nonzero in this block"'
    Bz, _ = t.gathered()
    ref, S = zs.reference(t.A, Bz, None, 1 + 0j, 0j)
    out = Cox.reshape(t.rows, t.ldx)
    tn = 64 if zs.INSTANTIATIONS[name][2] else zs.TILES[tile][1]
    worst = 0.0
    for z in range(batch):
        rows = t.tCo[z][t.tCo[z] >= 0]
        for j in range(nct):
            c0, c1 = 64 * j, min(N, 64 * j + 64)
            got = out[rows, c0:c1]
            if want[z, j] or tn < 64:
                worst = max(worst, zs.worst_ratio(got, ref[z][t.tCo[z] >= 0][:, c0:c1], S[z][t.tCo[z] >= 0][:, c0:c1], K))
            else:
                assert np.array_equal(got.copy().view(np.uint64), np.full_like(got, SENT).view(np.uint64)), 'an idle block was stored'
    check(worst, '%s [%s], sparse right-hand sides k2 %d' % (name, desc, k2))


# ---- 5. chunking of the batch at 65 535 items -----------------------------------------------------------------------------------------------------------
def test_chunked_launch_dense(helm_lib):
    rng = np.random.default_rng(3)
    batch = 70000
    p = Dense(rng, 8, 8, 8, batch, mixed=True)
    for alpha, beta in zs.ALPHA_BETA[1:]:
        w, rep = p.run(helm_lib, alpha, beta)
        check(w, 'chunked dense 8 x 8 x 8 x %d [tile %d slab %d]' % (batch, rep[0], rep[1]))


def test_chunked_launch_row_tables(helm_lib):
    """z0 enters the table row: item 65 535 + z of the second launch reads row 65 535 + z of the tables"""
    rng = np.random.default_rng(4)
    batch = 70000
    t = Table(rng, 8, 8, 8, batch, k2=3, ldx_pad=0, arena_rows=batch * 8 + 64)
    for alpha, beta, kw in ((-1 + 0j, 1 + 0j, {}), (0.3 - 0.2j, 0.5 + 0.1j, dict(second=True, oscale=0.6 - 1.3j))):
        w, rep = t.run(helm_lib, alpha, beta, **kw)
        check(w, 'chunked row-table 8 x 8 x 8 x %d [tile %d slab %d]' % (batch, rep[0], rep[1]))


# ---- 6. split over the inner dimension -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', sorted(zs.SPLITK, key=lambda s: -zs.SPLITK[s]), ids=lambda s: 'split%d-%dx%dx%dx%d' % ((zs.SPLITK[s],) + s))
def test_split_over_the_inner_dimension(helm_lib, shape):
    """factors 2 ... 16, K not divisible by the chunk, an empty last chunk, beta != 0 and ldc > N (k_splitk_reduce has its own addressing)"""
    M, N, K, batch = shape
    rng = np.random.default_rng(K + batch)
    p = Dense(rng, M, N, K, batch, pads=(3, 1, 61), gaps=(0, 9, 35), sa0=batch * M * K > (1 << 21), mixed=True)
    worst = 0.0
    for alpha, beta in zs.ALPHA_BETA:
        w, rep = p.run(helm_lib, alpha, beta)
        assert rep[:4] == (8, 8, 0, zs.SPLITK[shape]), rep
        assert w <= 1.0, (shape, alpha, beta, w)
        worst = max(worst, w)
    check(worst, 'split %d (chunk %d) of %s [tile 8 slab 8]' % (rep[3], rep[4], shape))
