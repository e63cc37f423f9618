"""GPU: the Krylov drivers of csrc/krylov.hip held to their recurrences, column by column, through helm_solve alone (no debug hook, no launch shape the
solver does not take): a helm_solve_opts of the test's own goes over ctypes, so that U and info are read also where columns end unconverged.

A. iterates    `maxit = k` makes the driver perform exactly k iterations; the returned iterate lies within 16 max(d_k, 64 u) of the extended-precision
               recurrence on the handle's own planes (tests/krylov_cases.py; d_k from the two CPU references, never from the device), info says what was
               done, relres is the true residual within a counted bound, a zero column comes back as zeros.
B. a column depends on nothing but itself: wavefield bits and info record are the same alone, at every position of a batch, beside a zero column, beside a
               column scaled by 1e6, beside columns that stop at other counts, across `batch` 0 and 3.  With method 'mg' at equal batch size and position.
C. polling changes nothing: check_every 1, 7, 50.
D. the refinement round (restart_masked, k_restart_copy, the masked branch of FIN_RESTART) on a batch where one column takes it and another does not.  Not
   covered: ST_PARKED and the un-park branch of FIN_RESTART, which only a restart after a breakdown inside run_bicgstab reaches."""
import ctypes

import numpy as np
import pytest

from tests import krylov_cases as kc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not kc.have_x87(), reason='numpy.longdouble is not the 80-bit format here')]

CAP_RTOL = 1e-30          # never met: a capped run stops at maxit alone
_OPS = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def operator(name, **kw):
    "one handle per case for the whole module"
    import zephyr_amd as za
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _OPS:
        cls = {'mz': za.MiniZephyr, 'eu': za.Eurus, 'tti': za.Eurus, '3d': za.Helm3D}[kc.CASES[name]['kind']]
        op = cls(kc.config(name, **kw))
        assert op.handle
        _OPS[key] = op
    return _OPS[key]


@pytest.fixture(scope='module', autouse=True)
def release_handles():
    yield
    for op in _OPS.values():
        del op.factors
    _OPS.clear()
    _PLANES.clear()


_PLANES = {}


def device_planes(lib, name):
    "the handle's own planes, as the references take them"
    from zephyr_amd import _lib
    if name not in _PLANES:
        op = operator(name)
        if kc.CASES[name]['kind'] == 'eu':
            out = np.empty((9,) + kc.CASES[name]['dims'], dtype=np.complex128)
            _lib.check(lib.helm_get_block_diagonals(op.handle, 0, _lib.ptr(out)), op.handle)
        else:
            out = op.diagonals()
            out = out[0] if kc.CASES[name]['kind'] == 'mz' else out
        _PLANES[name] = out
    return _PLANES[name]


def solve(lib, op, Q, premul=1.0 + 0j, method='bicgstab', maxit=200000, rtol=1e-9, check_every=0, batch=0):
    "helm_solve on the columns Q (ncol, rows): (U (ncol, rows), [(iterations, status, restarts, method, relres)])"
    from zephyr_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.complex128)
    ncol, rows = Q.shape
    U = np.full_like(Q, complex(np.nan, np.nan))
    info = (_lib.SolveInfo * ncol)()
    o = _lib.SolveOpts()
    o.method, o.rtol, o.maxit, o.check_every, o.batch, o.flags = _lib.METHODS[method], rtol, int(maxit), int(check_every), int(batch), 0
    pm = complex(premul)
    rc = lib.helm_solve(op.handle, _lib.ptr(Q), _lib.ptr(U), ncol, rows, pm.real, pm.imag, ctypes.byref(o), info)
    _lib.check(rc, op.handle)
    return U, [(i.iterations, i.status, i.restarts, i.method, i.relres) for i in info]


def record(U, info, j):
    "what must not depend on the rest of the batch: the bits of the wavefield and the info record (relres by its bits)"
    it, st, rs, me, rr = info[j]
    return bits(U[j]).tobytes(), (it, st, rs, me, float(rr).hex())


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------------
A_PARAMS = [(n, m, i) for n in kc.ITERATE_CASES for m in kc.case_methods(n) for i in range(len(kc.PREMULS))]


@pytest.mark.parametrize('name,method,ipm', A_PARAMS, ids=['%s-%s-premul%d' % p for p in A_PARAMS])
def test_iterates_follow_the_recurrence(helm_lib, name, method, ipm):
    """every k, column count and column: x_k = conj(U) within 16 max(d_k, 64 u) of x_k^exact, info = (k, 1, 0, method) [CGNR: k + 1, krylov_cases.cgnr_reported],
    relres within its counted bound (krylov_cases.relres_reference), the zero column exact zeros with (0, 0, 0, ., 0.0)"""
    from zephyr_amd import _lib
    lib, op, premul = helm_lib, operator(name), kc.PREMULS[ipm]
    C = kc.system_planes(name, device_planes(lib, name))
    ks, ncols = kc.case_ks(name), kc.case_ncols(name)
    Qmax, kinds = kc.rhs_columns(name, max(ncols))
    live = [j for j, kd in enumerate(kinds) if kd != 'zero']
    ex, d = kc.sensitivity(name, C, Qmax[live], premul, method, max(ks))
    fails, worst, worst_rr = [], 0.0, 0.0
    for ncol in ncols:
        Q, kd = kc.rhs_columns(name, ncol)
        assert np.array_equal(Q, Qmax[:ncol]) or ncol < 3
        for k in ks:
            want_it = kc.cgnr_reported(k) if method == 'cgnr' else k
            U, info = solve(lib, op, Q, premul, method, maxit=want_it, rtol=CAP_RTOL)
            nz = [j for j in range(ncol) if kd[j] != 'zero' and np.array_equal(Q[j], Qmax[j])]
            assert len(nz) == ncol - kd.count('zero')
            rr_ref, rr_bound = kc.relres_reference(name, C, Q[nz], premul, np.conj(U[nz]))
            for j in range(ncol):
                if kd[j] == 'zero':
                    if not (np.all(U[j] == 0) and info[j][:3] == (0, 0, 0) and info[j][4] == 0.0):
                        fails.append('ncol %d k %d: zero column %d came back %r, max |U| %g' % (ncol, k, j, info[j], np.abs(U[j]).max()))
                    continue
                pos = live.index(j)
                err = kc.relnorm(np.conj(U[j])[None], ex[k - 1][pos][None])[0]
                base = max(d[k - 1][pos], 64 * kc.U)
                worst = max(worst, err / base)
                if not err <= kc.MARGIN * base:
                    fails.append('ncol %d k %d column %d (%s): %.3e from x_k^exact, d_k %.3e, ratio %.1f' % (ncol, k, j, kd[j], err, d[k - 1][pos], err / base))
                if info[j][:4] != (want_it, 1, 0, _lib.METHODS[method]):
                    fails.append('ncol %d k %d column %d: info %r, expected (%d, 1, 0, %d)' % (ncol, k, j, info[j], want_it, _lib.METHODS[method]))
                i = nz.index(j)
                drr = abs(info[j][4] - rr_ref[i])
                worst_rr = max(worst_rr, drr / rr_bound[i])
                if not drr <= rr_bound[i]:
                    fails.append('ncol %d k %d column %d: relres %.17g, reference %.17g, bound %.3e' % (ncol, k, j, info[j][4], rr_ref[i], rr_bound[i]))
    print('A %s %s premul %s: worst error / max(d_k, 64 u) = %.2f (bound %g); worst |relres - reference| / bound = %.3f'
          % (name, method, premul, worst, kc.MARGIN, worst_rr))
    assert not fails, '\n'.join(fails)


# ---- B, C ------------------------------------------------------------------------------------------------------------------------------------------------
B_PARAMS = [('S', 'bicgstab'), ('M', 'bicgstab'), ('S', 'cgnr'), ('TTI', 'cgnr')]


class Registry(object):
    "the first record of every column; every later one must be the same"

    def __init__(self):
        self.first, self.diff = {}, []

    def see(self, key, U, info, j, where):
        rec = record(U, info, j)
        if key not in self.first:
            self.first[key] = (rec, where)
        elif self.first[key][0] != rec:
            (b0, i0), w0 = self.first[key]
            nb = int((np.frombuffer(b0, np.uint64) != np.frombuffer(rec[0], np.uint64)).sum())
            self.diff.append('column %r: %s gives info %r, %s gave %r; %d words of the wavefield differ' % (key, where, rec[1], w0, i0, nb))


@pytest.mark.parametrize('name,method', B_PARAMS)
def test_a_column_depends_on_nothing_but_itself(helm_lib, name, method):
    lib, op = helm_lib, operator(name)
    Q7, kinds = kc.rhs_columns(name, 7)
    reg = Registry()
    counts = None
    for t in (0, 1):                                    # a complex normal field, the point source
        U, info = solve(lib, op, Q7[[t]], method=method)
        reg.see(t, U, info, 0, 'alone')
        assert info[0][1] == 0, info
        # `iterations` is everything the column used, the rounds before a refinement included: that many suffice again, and give the same wavefield
        U, info = solve(lib, op, Q7[[t]], method=method, maxit=info[0][0])
        reg.see(t, U, info, 0, 'alone, maxit = the count it reported')
        if method == 'cgnr' and name == 'S':             # and not fewer than the double reference needs for the first round alone (two of slack for the roundings)
            _, steps = kc.cgnr_iterates(kc.System(name, kc.system_planes(name, device_planes(lib, name)), np.complex128), Q7[[t]], 1.0, 100000, rtol=0.5e-9)
            assert info[0][0] >= kc.cgnr_reported(steps) - 2, (info, steps)
        others = [j for j in range(5) if j != t]
        for pos in range(5):
            order = others[:pos] + [t] + others[pos:]
            U, info = solve(lib, op, Q7[order], method=method)
            for p, j in enumerate(order):
                reg.see(j, U, info, p, 'position %d of the batch %r' % (p, order))
            counts = {info[p][0] for p, j in enumerate(order) if kinds[j] != 'zero'}
            assert all(i[1] == 0 for i in info), info
        U, info = solve(lib, op, np.stack([Q7[t], np.zeros_like(Q7[t])]), method=method)
        reg.see(t, U, info, 0, 'beside a zero column')
        assert np.all(U[1] == 0) and info[1][:3] == (0, 0, 0) and info[1][4] == 0.0
        U, info = solve(lib, op, np.stack([1e6 * Q7[3], Q7[t]]), method=method)
        reg.see(t, U, info, 1, 'behind a column scaled by 1e6')
        reg.see('3 x 1e6', U, info, 0, 'scaled, first')
    for batch in (0, 3):                                # passes of 7, and of 3, 3, 1: the `first` offsets of rhs_b, sub_b, dXout
        U, info = solve(lib, op, Q7, method=method, batch=batch)
        for j in range(7):
            reg.see(j, U, info, j, '7 columns, batch = %d' % batch)
    for ce in (1, 7, 50):                               # C: the device, not the host poll, stops a column
        U, info = solve(lib, op, Q7[:5], method=method, check_every=ce)
        for j in range(5):
            reg.see(j, U, info, j, 'check_every = %d' % ce)
    print('B/C %s %s: iteration counts in the batch of five %r' % (name, method, sorted(counts)))
    assert len(counts) >= 2, 'the batch of five holds one iteration count only: %r' % (counts,)
    assert not reg.diff, '\n'.join(reg.diff)


@pytest.mark.parametrize('name,method', B_PARAMS)
def test_polling_changes_nothing_of_a_capped_run(helm_lib, name, method):
    lib, op = helm_lib, operator(name)
    Q, _ = kc.rhs_columns(name, 5)
    reg = Registry()
    for ce in (1, 7, 50):
        U, info = solve(lib, op, Q, kc.PREMULS[1], method, maxit=kc.cgnr_reported(8) if method == 'cgnr' else 8, rtol=CAP_RTOL, check_every=ce)
        for j in range(5):
            reg.see(j, U, info, j, 'check_every = %d' % ce)
    assert not reg.diff, '\n'.join(reg.diff)


# ---- B with the multigrid preconditioner: at equal batch size and position -------------------------------------------------------------------------------
def point_columns(dims, n, seed):
    rng = np.random.default_rng(seed)
    Q = np.zeros((n, int(np.prod(dims))), dtype=np.complex128)
    for s in range(n):
        at = tuple(int(rng.integers(2 if s % 3 else 8, d - 2)) for d in dims)        # (every third one may lie inside the absorbing layers)
        Q[s, int(np.ravel_multi_index(at, dims))] = complex(rng.standard_normal(), rng.standard_normal())
    return Q


def companions_do_not_matter(lib, op, dims, label):
    "the coarsest level is a GEMM whose shape follows the batch: the claim is at equal batch size and position -- exchanging the companions changes no bit"
    T = point_columns(dims, 2, 1)
    A = point_columns(dims, 4, 2)
    B = point_columns(dims, 4, 3)
    B[1] = 0
    B[2] *= 1e6
    diff, counts = [], []
    for t in range(2):
        for pos in (0, 2, 4):
            recs = []
            for comp in (A, B):
                Q = np.concatenate([comp[:pos], T[[t]], comp[pos:]])
                U, info = solve(lib, op, Q, method='mg', maxit=20000)
                assert info[pos][1] == 0, (label, info)
                recs.append(record(U, info, pos))
            counts.append(info[pos][0])
            if recs[0] != recs[1]:
                nb = int((np.frombuffer(recs[0][0], np.uint64) != np.frombuffer(recs[1][0], np.uint64)).sum())
                diff.append('%s: column %d at position %d: info %r against %r, %d words differ' % (label, t, pos, recs[0][1], recs[1][1], nb))
    assert not diff, '\n'.join(diff)
    return counts


def test_mg_companions_do_not_matter_2d(helm_lib):
    import zephyr_amd as za
    nz, nx = 72, 90
    rng = np.random.default_rng(7)
    op = za.MiniZephyr(dict(nx=nx, nz=nz, dx=10., dz=10., c=2000. + 800. * rng.random((nz, nx)), rho=1000. + 300. * rng.random((nz, nx)), freq=12., nPML=8))
    try:
        companions_do_not_matter(helm_lib, op, (nz, nx), '2-D 72 x 90')
    finally:
        del op.factors


def test_mg_companions_do_not_matter_3d(helm_lib, monkeypatch):
    """five columns on 30 x 26 x 28 under both hierarchies: HELM_MG3_KEEP = 2, the layer-preserving one (2: a hierarchy that cannot be built is an error, not a quiet
    fallback to the standard cycle), and 0, the standard shifted cycle.  HELM_MG3_DEPTH_MODEL = 0: the depth by the 10-points rule alone, not by timed set-ups.
    That the two ran different preconditioners is checked: their iteration counts differ, and the layer-preserving one stays below the 300 iterations at which
    the driver would retreat to the standard cycle."""
    import zephyr_amd as za
    dims = (30, 26, 28)
    iz = np.arange(dims[0])[:, None, None]
    c = (1800. + 25. * iz + 150. * (iz > 18)) * np.ones(dims)
    rho = 1000. + 300. * (iz > 18) * np.ones(dims)
    monkeypatch.setenv('HELM_MG3_DEPTH_MODEL', '0')
    its = {}
    for keep in ('2', '0'):
        monkeypatch.setenv('HELM_MG3_KEEP', keep)
        op = za.Helm3D(dict(nx=dims[2], ny=dims[1], nz=dims[0], dx=10., c=c, rho=rho, freq=4., nPML=6))
        try:
            its[keep] = companions_do_not_matter(helm_lib, op, dims, '3-D 30 x 26 x 28, HELM_MG3_KEEP=%s' % keep)
        finally:
            del op.factors
    print('B mg 3-D: iterations of the target columns, layer-preserving %r, standard cycle %r' % (its['2'], its['0']))
    assert max(its['2']) < 300 and its['2'] != its['0'], its


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refinement_round_on_part_of_a_batch(helm_lib):
    """case 'R', rtol = 1e-3: the point source on the smallest diagonal entry (column 3) meets the scaled criterion with its unscaled residual still above rtol
    and takes the refinement round -- restart_masked, k_restart_copy and the masked branch of FIN_RESTART; the point source in the middle of the grid (column 1)
    does not.  The CPU reference says so beforehand, by a factor of two either way; the device then reports restarts >= 1 on the one and 0 on the other, and every
    column has the bits and the info record it has alone.  Every other column has already stopped when this restart runs (run_bicgstab returns only when no
    column is active), so nothing is parked here: ST_PARKED and the un-park branch of FIN_RESTART are reached only by a restart after a breakdown inside
    run_bicgstab, which no test provokes -- they remain untested."""
    lib, op, rtol = helm_lib, operator('R'), kc.RESTART_RTOL
    C = device_planes(lib, 'R')
    Q, kinds = kc.restart_columns(C)
    takes, _ = kc.refinement_ratio('R', C, Q[3], rtol)
    spared, _ = kc.refinement_ratio('R', C, Q[1], rtol)
    assert takes > 2 and spared < 0.5, (takes, spared)
    U, info = solve(lib, op, Q, method='bicgstab', rtol=rtol)
    print('D: unscaled / rtol after the first round, from the CPU reference: column 3 %.2f, column 1 %.2f; device info %r' % (takes, spared, info))
    assert all(i[1] == 0 and i[4] <= rtol for i in info), info
    assert info[3][2] >= 1 and info[1][2] == 0, info
    reg = Registry()
    for j in range(5):
        reg.see(j, U, info, j, 'the batch of five')
    for j in (0, 1, 3, 4):
        Ua, ia = solve(lib, op, Q[[j]], method='bicgstab', rtol=rtol)
        reg.see(j, Ua, ia, 0, 'alone')
    for order in ([3, 1, 0, 4, 2], [1, 2, 4, 0, 3]):
        Uo, io = solve(lib, op, Q[order], method='bicgstab', rtol=rtol)
        for p, j in enumerate(order):
            reg.see(j, Uo, io, p, 'position %d of the batch %r' % (p, order))
    for ce, batch in ((1, 0), (7, 0), (50, 3)):
        Uo, io = solve(lib, op, Q, method='bicgstab', rtol=rtol, check_every=ce, batch=batch)
        for j in range(5):
            reg.see(j, Uo, io, j, 'check_every = %d, batch = %d' % (ce, batch))
    assert not reg.diff, '\n'.join(reg.diff)
