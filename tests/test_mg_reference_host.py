"""CPU: the reference of the 2-D multigrid preconditioner (tests/mg_cases.py) validated against itself -- the transfers are each other's transpose, Thomas
elimination agrees with dense solves of the tridiagonal systems cut out of the oracle's matrix, the cycle and M^-1 agree with the same operators written as
explicit scipy sparse matrices, every seeded mistake moves the reference by at least 1000 times the tolerance the GPU test (tests/test_gpu_mg_stage.py) uses for
that stage -- and the test hook helm_debug_mg_stage refuses malformed input before it touches a device."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import helm_oracle as ho
from tests import mg_cases as mc

pytestmark = pytest.mark.skipif(not mc.have_x87(), reason='numpy.longdouble is not the 80-bit format here')
LD, CLD = mc.LD, mc.CLD


def matrix_of(fn, shape_in):
    "the real matrix of a linear map on (1, nz, nx) arrays, column by column, in extended precision"
    n = int(np.prod(shape_in))
    cols = []
    for j in range(n):
        e = np.zeros(n, dtype=LD)
        e[j] = 1
        cols.append(fn(e.reshape((1,) + tuple(shape_in))).ravel())
    return np.stack(cols, axis=1)


@pytest.mark.parametrize('nzf,nxf', [(2, 2), (3, 3), (7, 8), (8, 7), (6, 6), (9, 9)])
def test_restriction_and_prolongation_are_transposes(nzf, nxf):
    "P = 4 R^T exactly (all weights are powers of two), odd and even dimensions in both axes; and the weights themselves at an interior and an edge point"
    nzc, nxc = mc.coarse_dims(nzf, nxf)
    R = matrix_of(mc.restrict, (nzf, nxf))
    P = matrix_of(lambda e: mc.prolong(e, nzf, nxf), (nzc, nxc))
    assert R.shape == (nzc * nxc, nzf * nxf) and P.shape == R.T.shape
    assert np.array_equal(P, 4 * R.T)
    assert R[0, 0] == 0.25 and (nxf < 2 or R[0, 1] == 0.125)                 # centre weight 4 / 16, edge neighbour 2 / 16: nothing is renormalised at the boundary
    if nzf >= 4 and nxf >= 4:
        assert np.array_equal(R[1 * nxc + 1].reshape(nzf, nxf)[1:4, 1:4], np.outer([1, 2, 1], [1, 2, 1]) / 16.0)


@pytest.mark.parametrize('kind,nz,nx', [('eurus', 17, 8), ('eurus', 8, 23), ('dominant', 17, 8), ('dominant', 8, 23)])
def test_thomas_against_dense_solves_of_the_oracle_matrix(kind, nz, nx):
    """u + wstrip T^-1 r with T cut out of the dense oracle matrix along every strip line (so the line geometry and the plane order are the oracle's, not
    line_systems') against line_relax; the bound 1e3 u cond(T) per line on the relative difference"""
    C, r, u, ex, _ = mc.line_case(kind, nz, nx, 2)
    W = mc.LINE_W
    A = mc.dense_of(C)
    idx = np.arange(nz * nx).reshape(nz, nx)
    lines = [idx[:, ix] for ix in list(range(W)) + list(range(nx - W, nx))] + [idx[iz, W:nx - W] for iz in list(range(W)) + list(range(nz - W, nz))]
    assert len(lines) == 4 * W and sum(len(ln) for ln in lines) == int(mc.on_lines(nz, nx, W).sum())
    got = np.asarray(ex).astype(np.complex128).reshape(2, -1)
    want = u.reshape(2, -1).copy()
    for ln in lines:
        T = A[np.ix_(ln, ln)]
        assert np.count_nonzero(np.triu(T, 2)) == 0 and np.count_nonzero(np.tril(T, -2)) == 0
        x = np.linalg.solve(T, r.reshape(2, -1)[:, ln].T).T
        want[:, ln] += mc.LINE_WSTRIP * x
        tol = 1e3 * mc.U * np.linalg.cond(T) * np.abs(x).max()
        assert np.abs(got[:, ln] - want[:, ln]).max() <= tol
    off = ~mc.on_lines(nz, nx, W).ravel()
    assert np.array_equal(got[:, off], u.reshape(2, -1)[:, off])


def test_thomas_factors_are_those_of_the_elimination():
    "m, cp, af of thomas_factors reproduce T: b_i = 1 / m_i + a_i cp_{i-1}, c_i = cp_i / m_i, a_i = -af_i / m_i"
    C = mc.cast(mc.line_planes('eurus', 21, 19), CLD)
    for a, b, c in mc.line_systems(C, 6):
        m, cp, af = mc.thomas_factors(a, b, c)
        prev = np.concatenate([np.zeros_like(cp[:, :1]), cp[:, :-1]], axis=1)
        for got, want in ((1 / m + a * prev, b), (cp / m, c), (-af / m, a)):
            assert np.abs(got - want).max() <= 64 * 2.0 ** -63 * np.abs(b).max()


# ---- the cycle as explicit sparse matrices -------------------------------------------------------------------------------------------------------------
def transfer_1d(nf):
    nc = (nf + 1) // 2
    R = sp.lil_matrix((nc, nf))
    for I in range(nc):
        for d, w in ((-1, 0.25), (0, 0.5), (1, 0.25)):
            if 0 <= 2 * I + d < nf:
                R[I, 2 * I + d] = w
    return R.tocsr()


class MatrixCycle(object):
    "the same preconditioner with every operator a scipy sparse matrix acting on (N, ncol) blocks, complex128"

    def __init__(self, levels, cinvT, strip, par):
        self.par = par
        self.A = [ho.coefficients_to_csr(C) for C, _ in levels]
        self.D = [sp.diags(par['omega_j'] * d.ravel()) for _, d in levels]
        self.R = [sp.kron(transfer_1d(C.shape[1]), transfer_1d(C.shape[2])).tocsr() for C, _ in levels[:-1]]
        self.Ainv = cinvT.T
        if strip is not None:
            nz, nx = strip.shape[1:]
            W = par['W']
            S = ho.coefficients_to_csr(strip).tocoo()
            on = mc.on_lines(nz, nx, W).ravel()
            zline = np.zeros((nz, nx), dtype=bool)
            zline[:, :W] = zline[:, nx - W:] = True
            zline = zline.ravel()
            iz, ix = np.divmod(S.row, nx)
            jz, jx = np.divmod(S.col, nx)
            same = np.where(zline[S.row], (ix == jx) & zline[S.col], (iz == jz) & on[S.col] & ~zline[S.col])
            keep = on[S.row] & same
            T = sp.coo_matrix((S.data[keep], (S.row[keep], S.col[keep])), shape=S.shape) + sp.diags((~on).astype(float))
            self.S, self.T, self.on = S.tocsr(), spla.splu(T.tocsc()), on

    def cycle(self, l, f, fmode):
        last = len(self.A) - 1
        if l == last:
            return self.Ainv @ f
        u = self.D[l] @ f
        for _ in range(self.par['nu1'] - 1):
            u = u + self.D[l] @ (f - self.A[l] @ u)
        fc = self.R[l] @ (f - self.A[l] @ u)
        e = self.cycle(l + 1, fc, fmode)
        if fmode and l < self.par['fdepth'] and l + 1 < last:
            e = e + self.cycle(l + 1, fc - self.A[l + 1] @ e, False)
        u = u + 4 * (self.R[l].T @ e)
        for _ in range(self.par['nu2']):
            u = u + self.D[l] @ (f - self.A[l] @ u)
        return u

    def apply(self, f):
        out = self.cycle(0, f, self.par['fdepth'] > 0)
        for _ in range(self.par['sweeps']):
            r = (f - self.S @ out) * self.on[:, None]
            out = out + self.par['wstrip'] * (self.T.solve(r) * self.on[:, None])
        return out


@pytest.mark.parametrize('name,over', [('eu70x67', {}), ('eu70x67', dict(nu1=2, nu2=2, fdepth=1)), ('eu20x40', {})])
def test_cycle_against_explicit_sparse_matrices(name, over):
    levels, cinvT, strip, par = mc.oracle_hier_inputs(name)
    par = dict(par, **over)
    assert len(levels) == (4 if name == 'eu70x67' else 1)      # (20 x 40 with ten layer cells stops at once: its cycle is the dense solve, and it has no strip)
    H = mc.Hier(levels, cinvT, strip, par, np.complex128)
    M = MatrixCycle(levels, cinvT, strip, par)
    for l in range(len(levels) - 1, -1, -1):
        F = mc.hier_rhs(name, levels[l][0].shape[1:])
        for fmode in (False, True):
            got = H.cycle(l, F, fmode).reshape(F.shape[0], -1)
            want = M.cycle(l, F.reshape(F.shape[0], -1).T, fmode).T
            assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max(), (l, fmode)
            assert np.all(got[-1] == 0)
    F = mc.hier_rhs(name, levels[0][0].shape[1:])
    got = H.apply(F).reshape(F.shape[0], -1)
    want = M.apply(F.reshape(F.shape[0], -1).T).T
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


# ---- seeded mistakes ----------------------------------------------------------------------------------------------------------------------------------------
def margin(exact, wrong, tol):
    "how many tolerances the mistake moves the result by (the largest over columns)"
    move = mc.colmax(np.asarray(wrong).astype(CLD) - exact)
    tol = np.asarray(tol, dtype=LD)
    return float((move[tol > 0] / tol[tol > 0]).max())


def test_seeded_mistakes_in_the_transfers():
    rng = np.random.default_rng(3)
    for nzf, nxf in [(7, 8), (17, 18), (35, 34)]:
        r = mc.crand(rng, 2, nzf, nxf)
        ex, bre, bim = mc.restrict_bounds(r)
        wrong = mc.restrict(mc.cast(r, CLD), mutant='restrict_edge')
        m = float(np.abs(wrong.real - ex.real).max() / bre.max())
        print('restriction edge weight on %d x %d: %.3g bounds' % (nzf, nxf, m))
        assert m >= 1000
        nzc, nxc = mc.coarse_dims(nzf, nxf)
        e, u = mc.crand(rng, 2, nzc, nxc), mc.crand(rng, 2, nzf, nxf)
        ex, bre, bim = mc.prolong_add_bounds(e, u)
        wrong = mc.cast(u, CLD) + mc.prolong(mc.cast(e, CLD), nzf, nxf, mutant='prolong_drop')
        m = float(np.abs(wrong.real - ex.real).max() / bre.max())
        print('prolongation without I + 1 on the last odd line of %d x %d: %.3g bounds' % (nzf, nxf, m))
        assert m >= 1000


@pytest.mark.parametrize('mutant', ['no_second_visit', 'omega_twice'])
def test_seeded_mistakes_in_the_cycle(mutant):
    name = 'eu70x67'
    levels, cinvT, strip, par = mc.oracle_hier_inputs(name)
    E, D, X = (mc.Hier(levels, cinvT, strip, par, dt, mu) for dt, mu in ((CLD, None), (np.complex128, None), (CLD, mutant)))
    F = mc.hier_rhs(name, levels[0][0].shape[1:])[:4]
    for what in ('cycle', 'apply'):
        run = (lambda h: h.cycle(0, F, True)) if what == 'cycle' else (lambda h: h.apply(F))
        ex = run(E)
        m = margin(ex, run(X), mc.floor_tol(ex, run(D)))
        print('%s, %s of level 0: %.3g tolerances' % (mutant, what, m))
        assert m >= 1000
    if mutant == 'no_second_visit':          # the second visit exists at two depths: level 1's own, seen from a cycle that starts there
        F1 = mc.hier_rhs(name, levels[1][0].shape[1:])[:4]
        ex = E.cycle(1, F1, True)
        m = margin(ex, X.cycle(1, F1, True), mc.floor_tol(ex, D.cycle(1, F1, True)))
        print('%s, cycle of level 1: %.3g tolerances' % (mutant, m))
        assert m >= 1000
        assert np.array_equal(E.cycle(2, mc.hier_rhs(name, levels[2][0].shape[1:]), True), X.cycle(2, mc.hier_rhs(name, levels[2][0].shape[1:]), True))


@pytest.mark.parametrize('kind', ['eurus', 'dominant'])
def test_seeded_mistake_in_the_line_solve(kind):
    "a carry dropped at point 1024, on every line length that has a second chunk, along z and along x"
    narrow = 2 * mc.LINE_W + 2
    for n in (1025, 2049, 2100):
        for nz, nx in ((n, narrow), (narrow, n + 2 * mc.LINE_W)):
            C, r, u, ex, tol = mc.line_case(kind, nz, nx, 1)
            wrong = mc.line_relax(mc.cast(C, CLD), mc.LINE_W, mc.cast(r, CLD), mc.cast(u, CLD), mc.LINE_WSTRIP, mutant='carry_1024')
            m = margin(ex, wrong, tol)
            print('carry dropped at 1024, %s %d x %d: %.3g tolerances' % (kind, nz, nx, m))
            assert m >= 1000


# ---- the hook refuses malformed input ------------------------------------------------------------------------------------------------------------------
def test_mg_stage_refuses_malformed_input_before_it_touches_a_device(helm_lib):
    z = lambda n: np.zeros(n, dtype=np.complex128)
    call = lambda stage, **a: mc.mg_stage(helm_lib, stage, **a)[0]
    ARG = mc.HELM_ERR_ARG
    assert helm_lib.helm_debug_mg_stage(None) == ARG
    assert call(99) == ARG and call(-1) == ARG
    assert call(mc.JAC0, nz=4, nx=4, nrhs=0, m=z(16), x=z(16), y=z(16)) == ARG
    assert call(mc.JAC0, nz=4, nx=4, nrhs=2, m=z(16), x=z(32), y=z(31)) == ARG
    assert call(mc.JAC0, nz=4, nx=4, nrhs=2, m=z(15), x=z(32), y=z(32)) == ARG
    assert call(mc.JAC0, nz=4, nx=4, nrhs=65, m=z(16), x=z(65 * 16), y=z(65 * 16)) == ARG
    assert call(mc.JAC0, nz=4, nx=4, nrhs=1, m=z(16), x=z(16), y=z(16), device=-1) == ARG
    assert call(mc.AXPY1, nz=4, nx=0, nrhs=1, x=z(16), y=z(16)) == ARG
    assert call(mc.RESTRICT, nz=5, nx=4, nrhs=1, x=z(20), y=z(5)) == ARG              # 3 x 2 coarse points
    assert call(mc.RESTRICT, nz=5, nx=4, nrhs=1, x=z(19), y=z(6)) == ARG
    assert call(mc.PROLONG_ADD, nz=5, nx=4, nrhs=1, x=z(5), y=z(20)) == ARG
    assert call(mc.PROLONG_ADD, nz=5, nx=4, nrhs=1, x=z(6), y=z(19)) == ARG
    assert call(mc.COARSE_DENSE, nz=5, nx=1, nrhs=1, m=z(24), x=z(5), y=z(5)) == ARG
    assert call(mc.COARSE_DENSE, nz=5, nx=2, nrhs=1, m=z(100), x=z(10), y=z(10)) == ARG
    assert call(mc.COARSE_DENSE, nz=4097, nx=1, nrhs=1, m=z(1), x=z(4097), y=z(4097)) == ARG
    lines = lambda n: [z(n), z(n), z(n)]
    assert call(mc.LINE_FACTOR, nz=8, nx=8, W=4, m=z(9 * 64), zl=lines(64), xl=lines(8)) == ARG            # 2 W + 2 > nz
    assert call(mc.LINE_FACTOR, nz=8, nx=8, W=3, m=z(9 * 64 - 1), zl=lines(48), xl=lines(12)) == ARG
    assert call(mc.LINE_FACTOR, nz=8, nx=8, W=3, m=z(9 * 64), zl=lines(47), xl=lines(12)) == ARG
    assert call(mc.LINE_FACTOR, nz=8, nx=8, W=3, m=z(9 * 64), zl=lines(48), xl=lines(11)) == ARG
    assert call(mc.LINE_FACTOR, nz=8, nx=8, W=3, m=z(9 * 64)) == ARG                                        # nowhere to put the factors
    assert call(mc.LINE_SOLVE, nz=8, nx=8, W=3, nrhs=1, m=z(9 * 64), r=z(63), y=z(64)) == ARG
    assert call(mc.LINE_SOLVE, nz=8, nx=8, W=3, nrhs=1, m=z(9 * 64), r=z(64), y=z(63)) == ARG
    assert call(mc.LINE_SOLVE, nz=8, nx=8, W=0, nrhs=1, m=z(9 * 64), r=z(64), y=z(64)) == ARG
    for stage in (mc.LEVELS, mc.PLANES, mc.STRIP_RESID, mc.CYCLE, mc.APPLY):                                  # no handle
        assert call(stage, nrhs=1, x=z(16), y=z(16), r=z(16)) == ARG
