"""GPU: the 2-D multigrid preconditioner of zephyr_amd/csrc/mg.hip, kernel by kernel and then composed, against the plain-numpy reference of tests/mg_cases.py in
numpy.clongdouble, through the test hook helm_debug_mg_stage (the kernels with the launch shapes vcycle / apply_typed give them).

Free-standing kernels: k_jac0, k_axpy1, k_restrict, k_prolong_add, k_coarse_dense, k_line_factor, k_line_solve -- the latter on line lengths of one lane, two
lanes, one full chunk of 1024 points, one point into a second chunk and three chunks, along z and along x, on the Eurus C-PML planes the strip exists for and on
a diagonally dominant set whose couplings carry 1000 points far.  Hierarchy: what mg_setup builds on five small grids, every cycle from the coarsest level up,
M^-1 with the solver's parameters and with nu1, nu2, fdepth, sweeps overridden, the tile-list residual, independence of the columns and masking.

Bounds: counted ones for JAC0, AXPY1 (bit for bit), RESTRICT, PROLONG_ADD, the strip residual; elsewhere 16 max(d, 64 u scale) with d from two CPU evaluations
(tests/mg_cases.py), never from the device.  Every test prints its worst error / bound.

Not covered: the single-precision storage (`P->f32`: k_convert, k_convert_rhs, the complex64 instantiations) and the fused stages (`P->fuse`: the xmode branches
of the stencil kernel), both hard-coded off in mg_setup, and the 3-D cycle (mg3*.hip)."""
import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import mg_cases as mc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not mc.have_x87(), reason='numpy.longdouble is not the 80-bit format here')]
LD, CLD = mc.LD, mc.CLD
_OPS, _HIER = {}, {}


def flat(a):
    return np.ascontiguousarray(a, dtype=np.complex128).ravel().copy()


def coef_close(got, ref, rtol=1e-13):
    "the tolerance tests/test_gpu_parity.py holds assembled planes to"
    scale = np.abs(ref).max()
    return np.abs(got - ref).max() <= rtol * scale * 50 and np.allclose(got, ref, rtol=1e-11, atol=1e-13 * scale)


def ok(rc, p=None):
    from zephyr_amd import _lib
    assert rc == 0, (rc, _lib.last_error(p.op if p is not None and p.op else None))


# ---- free-standing kernels ------------------------------------------------------------------------------------------------------------------------------
def batches():
    "(nrhs, active): one column; three with the middle one inactive"
    return [(1, None), (3, np.array([1, 0, 1], dtype=np.uint8))]


@pytest.mark.parametrize('nzf,nxf', mc.TRANSFER_GRIDS)
def test_transfers_and_vector_kernels(helm_lib, nzf, nxf):
    """RESTRICT and PROLONG_ADD (on a non-zero u) within their counted bounds, JAC0 within its, AXPY1 bit for bit the one rounding of a double addition; an
    inactive column comes back as it went in, bit for bit"""
    rng = np.random.default_rng(nzf * 1000 + nxf)
    nzc, nxc = mc.coarse_dims(nzf, nxf)
    worst = dict(restrict=0.0, prolong=0.0, jac0=0.0)
    for nrhs, act in batches():
        live = [j for j in range(nrhs) if act is None or act[j]]
        dead = [j for j in range(nrhs) if j not in live]
        r = mc.crand(rng, nrhs, nzf, nxf) * np.ldexp(1.0, rng.integers(-6, 7, size=(nrhs, 1, 1)))
        fc = np.full((nrhs, nzc, nxc), mc.SENT)
        y = flat(fc)
        ok(*mc.mg_stage(helm_lib, mc.RESTRICT, nz=nzf, nx=nxf, nrhs=nrhs, active=act, x=flat(r), y=y))
        y = y.reshape(fc.shape)
        ex, bre, bim = mc.restrict_bounds(r)
        worst['restrict'] = max(worst['restrict'], mc.ratio_parts(y[live], ex[live], bre[live], bim[live]))
        assert mc.same_bits(y[dead], fc[dead])

        e, u = mc.crand(rng, nrhs, nzc, nxc), mc.crand(rng, nrhs, nzf, nxf)
        y = flat(u)
        ok(*mc.mg_stage(helm_lib, mc.PROLONG_ADD, nz=nzf, nx=nxf, nrhs=nrhs, active=act, x=flat(e), y=y))
        y = y.reshape(u.shape)
        ex, bre, bim = mc.prolong_add_bounds(e, u)
        worst['prolong'] = max(worst['prolong'], mc.ratio_parts(y[live], ex[live], bre[live], bim[live]))
        assert mc.same_bits(y[dead], u[dead])

        dinv, f = mc.crand(rng, nzf, nxf), mc.crand(rng, nrhs, nzf, nxf)
        out = np.full(f.shape, mc.SENT)
        y = flat(out)
        ok(*mc.mg_stage(helm_lib, mc.JAC0, nz=nzf, nx=nxf, nrhs=nrhs, active=act, omega_j=0.8, m=flat(dinv), x=flat(f), y=y))
        y = y.reshape(f.shape)
        ex, bre, bim = mc.jac0_bounds(dinv, f, 0.8)
        worst['jac0'] = max(worst['jac0'], mc.ratio_parts(y[live], ex[live], bre[live], bim[live]))
        assert mc.same_bits(y[dead], out[dead])

        y = flat(u)
        ok(*mc.mg_stage(helm_lib, mc.AXPY1, nz=nzf, nx=nxf, nrhs=nrhs, active=act, x=flat(f), y=y))
        y = y.reshape(u.shape)
        assert mc.same_bits(y[live], (u + f)[live]) and mc.same_bits(y[dead], u[dead])
    print('transfers %d x %d: worst error / bound: restrict %.3f, prolong_add %.3f, jac0 %.3f; axpy1 bit for bit' % (nzf, nxf, worst['restrict'], worst['prolong'], worst['jac0']))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('nc', mc.COARSE_NCS)
def test_coarse_dense(helm_lib, nc):
    "u = invT^T f for a random invT: several workgroups per column share one LDS copy of f; three columns, the middle one inactive"
    invT, f, ex, tol = mc.coarse_case(nc)
    act = np.array([1, 0, 1], dtype=np.uint8)
    out = np.full(f.shape, mc.SENT)
    y = flat(out)
    ok(*mc.mg_stage(helm_lib, mc.COARSE_DENSE, nz=nc, nx=1, nrhs=3, active=act, m=flat(invT), x=flat(f), y=y))
    y = y.reshape(f.shape)
    ratio = mc.ratio_cols(y[[0, 2]], ex[[0, 2]], tol[[0, 2]])
    print('coarse_dense nc %d: worst error / bound %.3f' % (nc, ratio))
    assert ratio <= 1.0 and mc.same_bits(y[1], out[1])


@pytest.mark.parametrize('W', [3, 6])
def test_line_factor(helm_lib, W):
    "m, cp, af of every z-line and x-line against the recurrences in extended precision, line by line"
    nz, nx = 21, 19
    C = mc.line_planes('eurus', nz, nx)
    zl = [np.full(2 * W * nz, mc.SENT) for _ in range(3)]
    xl = [np.full(2 * W * (nx - 2 * W), mc.SENT) for _ in range(3)]
    ok(*mc.mg_stage(helm_lib, mc.LINE_FACTOR, nz=nz, nx=nx, W=W, m=flat(C), zl=zl, xl=xl))
    worst = 0.0
    for got, sys_e, sys_d in zip((zl, xl), mc.line_systems(mc.cast(C, CLD), W), mc.line_systems(C, W)):
        for g, e, d in zip(got, mc.thomas_factors(*sys_e), mc.thomas_factors(*sys_d)):
            worst = max(worst, mc.ratio_cols(g.reshape(e.shape), e, mc.floor_tol(e, d)))
    print('line_factor W %d: worst error / bound %.3f' % (W, worst))
    assert worst <= 1.0


LINE_PARAMS = [(k, nz, nx) for k in ('eurus', 'dominant') for nz, nx in mc.line_grids()]


@pytest.mark.parametrize('kind,nz,nx', LINE_PARAMS, ids=['%s-%dx%d' % p for p in LINE_PARAMS])
def test_line_solve(helm_lib, kind, nz, nx):
    """k_line_factor + k_line_solve: u + wstrip T^-1 r on every strip line within 16 max(d, 64 u scale) per column, u outside the lines and the inactive
    column bit for bit unchanged; one column, and five with column 2 inactive.  Lines of more than 1024 points carry a value between chunks: on the dominant
    set the reference itself moves by far more than the tolerance at the far end of the line when that carry is dropped."""
    W = mc.LINE_W
    on = mc.on_lines(nz, nx, W)
    worst = 0.0
    for ncol in (1, 5):
        C, r, u, ex, tol = mc.line_case(kind, nz, nx, ncol)
        act = None if ncol == 1 else np.array([1, 1, 0, 1, 1], dtype=np.uint8)
        live = [j for j in range(ncol) if act is None or act[j]]
        y, rr = flat(u), flat(r)
        ok(*mc.mg_stage(helm_lib, mc.LINE_SOLVE, nz=nz, nx=nx, W=W, nrhs=ncol, active=act, wstrip=mc.LINE_WSTRIP, m=flat(C), r=rr, y=y))
        y = y.reshape(u.shape)
        worst = max(worst, mc.ratio_cols(y[live], ex[live], tol[live]))
        assert mc.same_bits(y[:, ~on], u[:, ~on]), 'u outside the lines changed'
        if act is not None:
            assert mc.same_bits(y[2], u[2]) and mc.same_bits(rr.reshape(r.shape)[2], r[2]), 'the inactive column changed'
    if kind == 'dominant' and max(nz, nx - 2 * W) == 2100:
        C, r, u, ex, tol = mc.line_case(kind, nz, nx, 1)
        wrong = mc.line_relax(mc.cast(C, CLD), W, mc.cast(r, CLD), mc.cast(u, CLD), mc.LINE_WSTRIP, mutant='carry_1024')
        far = (np.abs(wrong - ex)[0, -10:, :W] if nz == 2100 else np.abs(wrong - ex)[0, :W, -10 - W:-W]).max()
        print('line_solve %s %d x %d: a carry dropped at point 1024 moves the last ten points by %.3g tolerances' % (kind, nz, nx, far / tol[0]))
        assert far >= 1000 * tol[0]
    print('line_solve %s %d x %d: worst error / bound %.3f' % (kind, nz, nx, worst))
    assert worst <= 1.0


# ---- hierarchy ---------------------------------------------------------------------------------------------------------------------------------------------
HIER = list(mc.HIER_CASES)
NB = 5


def operator(name, **kw):
    "one handle per case for the whole module"
    import zephyr_amd as za
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _OPS:
        cls = {'mz': za.MiniZephyr, 'eu': za.Eurus}[mc.HIER_CASES[name]['kind']]
        op = cls(dict(mc.hier_config(name), **kw))
        assert op.handle
        _OPS[key] = op
    return _OPS[key]


@pytest.fixture(scope='module', autouse=True)
def release_handles():
    yield
    for op in _OPS.values():
        del op.factors
    _OPS.clear()
    _HIER.clear()


class DeviceHier(object):
    "what the handle's own hierarchy holds, downloaded once: LEVELS, the planes and dinv of every level, cinvT, the strip operator with its line factors"

    def __init__(self, lib, op):
        self.h = op.handle
        tiles = np.full(1 << 16, -1, dtype=np.int32)
        rc, p = mc.mg_stage(lib, mc.LEVELS, op=self.h, nrhs=NB, tiles=tiles)
        ok(rc, p)
        self.info = p
        self.nl = p.nlevels
        self.grids = [(p.lev_nz[l], p.lev_nx[l], p.lev_dx[l], p.lev_dz[l], p.lev_npml[l]) for l in range(self.nl)]
        self.tiles = tiles[:p.o_ntiles].copy()
        self.par = dict(W=p.o_W, sweeps=p.o_sweeps, nu1=p.o_nu1, nu2=p.o_nu2, fdepth=p.o_fdepth, omega_j=p.o_omega_j, wstrip=p.o_wstrip)
        self.levels = []
        self.cinvT = np.full(p.o_nc * p.o_nc, mc.SENT)
        for l in range(self.nl):
            nz, nx = self.grids[l][:2]
            C, d = np.full(9 * nz * nx, mc.SENT), np.full(nz * nx, mc.SENT)
            ok(*mc.mg_stage(lib, mc.PLANES, op=self.h, level=l, y=C, r=d, cinvT=self.cinvT if l == 0 else None))
            self.levels.append((C.reshape(9, nz, nx), d.reshape(nz, nx)))
        self.cinvT = self.cinvT.reshape(p.o_nc, p.o_nc)
        self.strip = self.zl = self.xl = None
        nz, nx = self.grids[0][:2]
        W = p.o_W
        if p.o_sweeps > 0:
            S = np.full(9 * nz * nx, mc.SENT)
            self.zl = [np.full(2 * W * nz, mc.SENT) for _ in range(3)]
            self.xl = [np.full(2 * W * (nx - 2 * W), mc.SENT) for _ in range(3)]
            ok(*mc.mg_stage(lib, mc.PLANES, op=self.h, level=-1, y=S, zl=self.zl, xl=self.xl))
            self.strip = S.reshape(9, nz, nx)
        else:
            rc, _ = mc.mg_stage(lib, mc.PLANES, op=self.h, level=-1, y=np.zeros(9 * nz * nx, dtype=np.complex128))
            assert rc == mc.HELM_ERR_STATE
        self.exact = mc.Hier(self.levels, self.cinvT, self.strip, self.par, CLD)
        self.double = mc.Hier(self.levels, self.cinvT, self.strip, self.par, np.complex128)


def device_hier(lib, name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _HIER:
        _HIER[key] = DeviceHier(lib, operator(name, **kw))
    return _HIER[key]


def run(lib, H, stage, F, out=None, active=None, **kw):
    "a batched hierarchy stage on F (ncol, nz, nx): the output (same shape), which went up as `out` (default: the sentinel everywhere)"
    y = flat(np.full(F.shape, mc.SENT) if out is None else out)
    rc, p = mc.mg_stage(lib, stage, op=H.h, nrhs=F.shape[0], x=flat(F), y=y, active=active, **kw)
    ok(rc, p)
    return y.reshape(F.shape)


@pytest.mark.parametrize('name', HIER)
def test_construction(helm_lib, name):
    """what mg_setup built: the levels by its rules, the shifted tau and the weak layer, level and strip planes against the oracle's coefficients for that
    level's grid and injected model (MiniZephyr: outside the absorbing layer, where pml_scale does not reach), dinv the floored reciprocal, cinvT the inverse
    of the coarsest matrix, the line factors of the strip, the tile list"""
    cs = mc.HIER_CASES[name]
    op = operator(name)
    H = device_hier(helm_lib, name)
    p = H.info
    want = mc.level_rules(cs['dims'][0], cs['dims'][1], cs['h'][1], cs['h'][0], cs['nPML'])
    assert H.grids == want, (H.grids, want)
    if name == 'eu70x67':
        assert [g[:2] for g in H.grids] == [(70, 67), (35, 34), (18, 17), (9, 9)]
    assert H.nl >= 4 or name == 'eu20x40'           # (20 x 40 with ten layer cells: mg_setup's stopping rule leaves the one level, solved densely)
    par = mc.solver_par(name)
    assert H.par == par, (H.par, par)
    assert p.o_beta == mc.BETA and p.o_nc == H.grids[-1][0] * H.grids[-1][1]
    tau = mc.shifted_tau(cs['freq'], float(op.tau))
    assert abs(p.o_tau - tau) <= 4 * mc.U * tau
    assert p.o_cpml == (mc.CPML_WEAK if cs['kind'] == 'eu' else 0.0)

    worst_dinv = 0.0
    for l, (C, dinv) in enumerate(H.levels):
        nz, nx, _, _, npml = H.grids[l]
        ref = mc.oracle_level_planes(name, mc.CPML_WEAK, l, tau=p.o_tau)
        if cs.get('transposed'):
            ref = ac.transpose_planes(ref)
        if cs['kind'] == 'eu':
            assert coef_close(C, ref), (name, l)
        else:
            inner = (slice(None), slice(npml + 1, nz - npml - 1), slice(npml + 1, nx - npml - 1))
            assert C[inner].size > 0 and coef_close(C[inner], ref[inner]), (name, l)
        # dinv: the row's absolute sum (nine moduli of 4 roundings, 8 additions), the quotient and the scaling (4), Smith's reciprocal (6): gamma_32 |dinv| covers it
        exd = mc.dinv_floored(C, mc.DIAG_FLOOR)
        derr, dbound = np.abs(dinv.astype(CLD) - exd), mc.gamma(32) * np.abs(exd)
        assert np.all(derr[dbound == 0] == 0), (name, l)
        worst_dinv = max(worst_dinv, float((derr[dbound > 0] / dbound[dbound > 0]).max()))
    print('construction %s: dinv against the floored reciprocal, worst error / bound %.3f' % (name, worst_dinv))
    assert worst_dinv <= 1.0
    if H.strip is not None:
        # (the strip operator of both classes carries the true layer: MiniZephyr's pml_scale stays 1 on it)
        ref = mc.oracle_level_planes(name, 1e3, 0, tau=p.o_tau)
        assert coef_close(H.strip, ac.transpose_planes(ref) if cs.get('transposed') else ref), name
        worst = 0.0
        for got, sys_e, sys_d in zip((H.zl, H.xl), mc.line_systems(mc.cast(H.strip, CLD), p.o_W), mc.line_systems(H.strip, p.o_W)):
            for g, e, d in zip(got, mc.thomas_factors(*sys_e), mc.thomas_factors(*sys_d)):
                worst = max(worst, mc.ratio_cols(g.reshape(e.shape), e, mc.floor_tol(e, d)))
        print('construction %s: line factors of the strip, worst error / bound %.3f' % (name, worst))
        assert worst <= 1.0

    # cinvT^T A_c = I, as well as numpy's float64 inverse of the same matrix manages (the larger of its two residuals, times 16); products in extended
    # precision up to 256 unknowns, in double for both inverses alike beyond
    A = mc.dense_of(H.levels[-1][0])
    dt = CLD if A.shape[0] <= 256 else np.complex128
    Ae, I = A.astype(dt), np.eye(A.shape[0])
    inv = np.linalg.inv(A).astype(dt)
    bound = 16 * max(np.abs(inv @ Ae - I).max(), np.abs(Ae @ inv - I).max())
    got = np.abs(H.cinvT.T.astype(dt) @ Ae - I).max()
    print('construction %s: |cinvT^T A - I| %.3g, bound %.3g, ratio %.3f' % (name, got, bound, got / bound))
    assert got <= bound

    # the tile list: every 64 x tile_rows stencil tile that holds a point of the frame of width W, none twice
    nz, nx = cs['dims']
    if par['sweeps']:
        TZ, W = p.o_tile_rows, p.o_W
        ntx = (nx + 63) // 64
        frame = mc.on_lines(nz, nx, W)
        expect = sorted({(iz // TZ) * ntx + ix // 64 for iz, ix in zip(*np.nonzero(frame))})
        assert len(set(H.tiles.tolist())) == len(H.tiles) and sorted(H.tiles.tolist()) == expect
    else:
        assert p.o_ntiles == 0


def test_levels_of_the_transposed_handle_are_the_transposed_levels(helm_lib):
    """bit for bit, level by level, and the strip operator's planes too.  (dinv is not compared: its floor goes by the absolute sum of a row, and the rows of A^T
    are the columns of A; test_construction holds the transposed handle's dinv to its own planes.)"""
    T = device_hier(helm_lib, 'mz70x67T')
    P = device_hier(helm_lib, 'mz70x67T', transposed=False)
    assert helm_lib.helm_get_transposed(T.h) == 1 and helm_lib.helm_get_transposed(P.h) == 0
    assert T.grids == P.grids and T.nl >= 4
    for (Ct, _), (Cp, _) in zip(T.levels, P.levels):
        assert mc.same_bits(Ct, ac.transpose_planes(Cp)) and not mc.same_bits(Ct, Cp)
    assert mc.same_bits(T.strip, ac.transpose_planes(P.strip))


@pytest.mark.parametrize('name', HIER)
def test_composition(helm_lib, name):
    """CYCLE from the coarsest level up to level 0, with fmode off and on, then APPLY: four random columns and a zero one (which must give zeros) against the
    reference on the handle's own planes"""
    H = device_hier(helm_lib, name)
    worst, fails = {}, []
    for l in range(H.nl - 1, -1, -1):
        F = mc.hier_rhs(name, H.grids[l][:2])
        for fmode in (0, 1):
            got = run(helm_lib, H, mc.CYCLE, F, level=l, fmode=fmode)
            ex = H.exact.cycle(l, F, bool(fmode))
            tol = mc.floor_tol(ex, H.double.cycle(l, F, bool(fmode)))
            worst[(l, fmode)] = mc.ratio_cols(got[:4], ex[:4], tol[:4])
            if not np.all(got[4] == 0):
                fails.append('level %d fmode %d: the zero column came back with max |u| %g' % (l, fmode, np.abs(got[4]).max()))
    F = mc.hier_rhs(name, H.grids[0][:2])
    got = run(helm_lib, H, mc.APPLY, F)
    ex = H.exact.apply(F)
    worst['apply'] = mc.ratio_cols(got[:4], ex[:4], mc.floor_tol(ex, H.double.apply(F))[:4])
    if not np.all(got[4] == 0):
        fails.append('apply: the zero column came back with max |u| %g' % np.abs(got[4]).max())
    print('composition %s: worst error / bound by (level, fmode): %s' % (name, ', '.join('%s %.3f' % (k, v) for k, v in worst.items())))
    fails += ['%s: error / bound %.3f' % (k, v) for k, v in worst.items() if not v <= 1.0]
    assert not fails, '\n'.join(fails)


OVERRIDES = [dict(nu1=a, nu2=b) for a, b in ((1, 1), (2, 1), (1, 2), (2, 2))] + [dict(fdepth=d) for d in (0, 1, 3)] + [dict(sweeps=s) for s in (0, 1, 4)]


@pytest.mark.parametrize('name', HIER)
def test_overrides(helm_lib, name):
    """APPLY with (nu1, nu2), fdepth and sweeps overridden for the call: both parities of the ping-pong start, the V-cycle, one and three levels of second
    visits, no / one / four strip sweeps; afterwards the solver's own values are in force again.  Where the strip is off, sweeps > 0 is refused."""
    H = device_hier(helm_lib, name)
    F = mc.hier_rhs(name, H.grids[0][:2])
    base = run(helm_lib, H, mc.APPLY, F)
    worst, fails = {}, []
    for over in OVERRIDES:
        key = ' '.join('%s=%d' % kv for kv in over.items())
        if over.get('sweeps', 0) > 0 and H.strip is None:
            rc, _ = mc.mg_stage(helm_lib, mc.APPLY, op=H.h, nrhs=F.shape[0], x=flat(F), y=flat(F), **over)
            assert rc == mc.HELM_ERR_STATE, (key, rc)
            continue
        got = run(helm_lib, H, mc.APPLY, F, **over)
        ex = H.exact.with_par(**over).apply(F)
        tol = mc.floor_tol(ex, H.double.with_par(**over).apply(F))
        worst[key] = mc.ratio_cols(got[:4], ex[:4], tol[:4])
        if not np.all(got[4] == 0):
            fails.append('%s: the zero column came back with max |u| %g' % (key, np.abs(got[4]).max()))
    assert mc.same_bits(run(helm_lib, H, mc.APPLY, F), base), 'an override outlived its call'
    print('overrides %s: worst error / bound: %s' % (name, ', '.join('%s %.3f' % kv for kv in worst.items())))
    fails += ['%s: error / bound %.3f' % kv for kv in worst.items() if not kv[1] <= 1.0]
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('name', HIER)
def test_strip_residual(helm_lib, name):
    """the tile-list residual launch of one sweep: in - A_strip out on every point of every listed tile within 24 u (|in| + sum |c_k| |out_k|) in moduli (nineteen
    terms per component, products rounded once or twice: the bound of tests/resid_cases.py); every other point and the inactive column as they went in"""
    H = device_hier(helm_lib, name)
    nz, nx = H.grids[0][:2]
    rng = np.random.default_rng(77)
    IN, OUT = mc.crand(rng, 3, nz, nx), mc.crand(rng, 3, nz, nx)
    act = np.array([1, 0, 1], dtype=np.uint8)
    if H.strip is None:
        rc, _ = mc.mg_stage(helm_lib, mc.STRIP_RESID, op=H.h, nrhs=3, x=flat(IN), r=flat(OUT), y=flat(IN * 0), active=act)
        assert rc == mc.HELM_ERR_STATE
        return
    got = run(helm_lib, H, mc.STRIP_RESID, IN, r=flat(OUT), active=act)
    ex = H.exact.strip_resid(IN, OUT)
    S = np.abs(IN).astype(LD) + mc.stencil(np.abs(H.strip).astype(LD), np.abs(OUT).astype(LD))
    TZ, ntx = H.info.o_tile_rows, (nx + 63) // 64
    tile_of = (np.arange(nz)[:, None] // TZ) * ntx + np.arange(nx)[None, :] // 64
    listed = np.isin(tile_of, H.tiles)
    assert listed[mc.on_lines(nz, nx, H.info.o_W)].all()
    err = np.abs(got.astype(CLD) - ex)[[0, 2]][:, listed]
    ratio = float((err / (24 * mc.U * S[[0, 2]][:, listed])).max())
    print('strip residual %s: %d of %d tiles listed, worst error / bound %.3f' % (name, len(H.tiles), ntx * ((nz + TZ - 1) // TZ), ratio))
    assert ratio <= 1.0
    assert np.all(got[[0, 2]][:, ~listed] == mc.SENT) and np.all(got[1] == mc.SENT)


@pytest.mark.parametrize('name', HIER)
def test_independence_and_masking(helm_lib, name):
    """the bits of M^-1 of a column are the same alone, at each position of a batch of five and beside an inactive column; an inactive column's output comes back
    as the sentinel it went in with, whatever its input holds"""
    H = device_hier(helm_lib, name)
    F = mc.hier_rhs(name, H.grids[0][:2], ncol=NB, seed=1)[:NB]
    F[3] *= 1e6
    for t in (0, 1):
        alone = run(helm_lib, H, mc.APPLY, F[[t]])[0]
        assert np.all(np.isfinite(alone)) and np.abs(alone).max() > 0
        others = [j for j in range(NB) if j != t]
        for pos in range(NB):
            order = others[:pos] + [t] + others[pos:]
            got = run(helm_lib, H, mc.APPLY, F[order])
            assert mc.same_bits(got[pos], alone), 'column %d at position %d of %r' % (t, pos, order)
        pair = np.stack([F[t], np.full_like(F[t], np.nan)])
        got = run(helm_lib, H, mc.APPLY, pair, active=np.array([1, 0], dtype=np.uint8))
        assert mc.same_bits(got[0], alone) and np.all(got[1] == mc.SENT)
        got = run(helm_lib, H, mc.APPLY, pair[::-1].copy(), active=np.array([0, 1], dtype=np.uint8))
        assert mc.same_bits(got[1], alone) and np.all(got[0] == mc.SENT)
    for l in range(H.nl):                      # and of every cycle: columns 1 and 3 of five inactive
        Fl = mc.hier_rhs(name, H.grids[l][:2], ncol=NB, seed=2)[:NB]
        act = np.array([1, 0, 1, 0, 1], dtype=np.uint8)
        full = run(helm_lib, H, mc.CYCLE, Fl, level=l, fmode=1)
        got = run(helm_lib, H, mc.CYCLE, Fl, level=l, fmode=1, active=act)
        assert mc.same_bits(got[[0, 2, 4]], full[[0, 2, 4]]) and np.all(got[[1, 3]] == mc.SENT), 'level %d' % l
