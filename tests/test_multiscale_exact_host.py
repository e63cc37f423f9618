"""CPU: the exact transpose of the grid transfer.  helm_regrid_axis_t (host only) against the dense transpose of helm_regrid_axis, entry for
entry; `ds.matrix` against the Kronecker product of the dense axes; `ds.adjoint` against `ds.matrix.T`; and that `ds.T`, the interpolation
back up, is something else."""
import numpy as np
import pytest
from scipy.interpolate import make_interp_spline

from tests.multiscale_exact_cases import AXIS_PAIRS, GRID_PAIRS, dense_axis, dense_axis_t, dense_axes, interpolator, touched_width


@pytest.mark.parametrize('n_in,n_out,h_out', AXIS_PAIRS)
def test_transposed_axis_is_the_dense_transpose(helm_lib, n_in, n_out, h_out):
    from zephyr_amd import _lib
    M, W = dense_axis(n_in, 1., n_out, h_out)
    wt = touched_width(M)
    print('axis %d -> %d (h_out %.4g): W = %d, WT = %d' % (n_in, n_out, h_out, W, wt))
    if h_out >= 1.:
        assert wt <= 64
    if wt > 64:                                    # (an up-sampling axis: more than 64 outputs read one input node)
        assert h_out < 1.
        assert helm_lib.helm_regrid_axis_t(n_in, 1., n_out, h_out, None, None, 0) == -4          # HELM_ERR_UNSUPPORTED
        assert 'more than 64' in _lib.last_error()
        with pytest.raises(NotImplementedError):
            dense_axis_t(n_in, 1., n_out, h_out)
        return
    MT, start, WT = dense_axis_t(n_in, 1., n_out, h_out)          # (asserts every window in bounds)
    assert WT == wt
    assert np.array_equal(MT, M.T)                                # the same doubles, only moved
    # a node no output touches has an all-zero window
    for j in np.nonzero(~M.any(axis=0))[0]:
        assert not MT[j].any()


def test_unsupported_up_sampling_axis(helm_lib):
    assert helm_lib.helm_regrid_axis_t(10, 1., 100, 0.1, None, None, 0) == -4
    assert helm_lib.helm_regrid_axis_t(3, 1., 5, 0.5, None, None, 0) == -1                        # (too short for a cubic: as helm_regrid_axis)


def test_transposed_axis_needs_room_for_its_taps(helm_lib):
    from zephyr_amd import _lib
    start = np.zeros(57, dtype=np.int32)
    taps = np.zeros(10)
    assert helm_lib.helm_regrid_axis_t(57, 1., 20, 2.9, _lib.ptr(start), _lib.ptr(taps), taps.size) == -1


@pytest.mark.parametrize('name,shape,scale,target', GRID_PAIRS, ids=[g[0] for g in GRID_PAIRS])
@pytest.mark.parametrize('eCons', [False, True])
def test_matrix_is_the_kronecker_product_and_adjoint_its_transpose(helm_lib, name, shape, scale, target, eCons):
    ds = interpolator(shape, scale, target, eCons=eCons, hostTransfer=True)
    if target is not None:
        assert (ds.snz, ds.snx) == target
    Az, Ax, _, _ = dense_axes(ds)
    S = ds.matrix
    assert S.shape == ds.shape
    gain = scale ** 2 if (eCons and not ds.identity) else 1.
    assert np.array_equal(S.toarray(), gain * np.kron(Az, Ax))
    adj = ds.adjoint
    assert adj.shape == (ds.shape[1], ds.shape[0]) and adj.adjoint is ds and ds.adjoint is adj
    assert adj.gain == ds.gain
    rng = np.random.default_rng(4)
    for g in (rng.standard_normal(ds.shape[0]), rng.standard_normal((ds.shape[0], 3)) + 1j * rng.standard_normal((ds.shape[0], 3))):
        out = adj * g
        assert out.shape == (ds.shape[1],) + g.shape[1:] and out.dtype == g.dtype
        assert np.array_equal(out, S.T @ g)
    f = rng.standard_normal((ds.shape[1], 2)) + 1j * rng.standard_normal((ds.shape[1], 2))
    assert np.array_equal(ds * f, S @ f)                          # hostTransfer: `*` by the same matrix
    assert (ds * f[:, 0].real).dtype == np.float64
    if not ds.identity:
        with pytest.raises(ValueError):
            adj * np.zeros(ds.shape[1])


def test_adjoint_without_a_gpu_is_the_matrix_transpose(helm_lib, monkeypatch):
    from zephyr_amd import _lib
    monkeypatch.setattr(_lib, 'gpu_usable', lambda: False)
    ds = interpolator((40, 57), 2.47, (17, 23))                   # (no hostTransfer key)
    g = np.random.default_rng(2).standard_normal(ds.shape[0])
    assert np.array_equal(ds.adjoint * g, ds.matrix.T @ g)


def test_column_sums_show_sampling_not_averaging(helm_lib):
    M, _ = dense_axis(48, 1., 19, 2.47)
    sums = M.sum(axis=0)
    print('column sums of 48 -> 19 at 2.47: %.3f .. %.3f' % (sums.min(), sums.max()))
    assert abs(sums.min() + 0.25) < 0.01 and abs(sums.max() - 1.07) < 0.01
    M4, _ = dense_axis(30, 1., 8, 4.)
    hit = np.nonzero(M4.any(axis=0))[0]
    assert np.array_equal(hit, 4 * np.arange(8))                  # an integer scale: only every s-th node receives anything


def scipy_axis(n_in, n_out, h_out):
    x = np.arange(n_in, dtype=float)
    p = np.clip(np.arange(n_out) * h_out, x[0], x[-1])
    return make_interp_spline(x, np.eye(n_in), k=3)(p)


def test_the_upscaler_is_not_the_adjoint(helm_lib):
    """`ds.T` interpolates back up; the adjoint is the transpose of the down-scaler.  Their relative difference is of order 1, in scipy's own
    arithmetic (the reference alone) and in the project's matrices."""
    nz, nx, snz, snx, s = 40, 48, 17, 21, 2.31
    down = np.kron(scipy_axis(nz, snz, s), scipy_axis(nx, snx, s))
    up = np.kron(scipy_axis(snz, nz, 1. / s), scipy_axis(snx, nx, 1. / s))
    miss_ref = np.linalg.norm(up - down.T) / np.linalg.norm(down.T)
    ds = interpolator((nz, nx), s, (snz, snx))
    A = ds.matrix.T.toarray()
    miss = np.linalg.norm(ds.T.matrix.toarray() - A) / np.linalg.norm(A)
    print('|up - down^T| / |down^T|: scipy %.3f, zephyr_amd %.3f' % (miss_ref, miss))
    assert miss_ref >= 0.1 and miss >= 0.1
    assert np.abs(ds.matrix.toarray() - down).max() <= 1e-13


# ---- the exact derivatives of a multiscale pairing, numpy routes on the oracle doubles ----------------------------------------------------------------
from tests import adjoint_cases as ac                     # noqa: E402
from tests import multiscale_exact_cases as mc            # noqa: E402

FULL, OP = dict(linearisation='full'), dict(linearisation='operator')
KEYS = [(case, mode) for case in mc.PROBLEM_CASES for mode in ('fixed', 'relative')]
KEY_IDS = ['%s-%s' % k for k in KEYS]


@pytest.fixture(scope='module')
def solved(helm_lib):
    'per (case, mode, density): the pair, its config and the per-grid host fields -- made once and left unchanged'
    out = {}
    for case, mode in KEYS:
        for density in (True, False):
            prob, sv, sc = mc.host_pair(case, mode, density=density)
            out[(case, mode, density)] = dict(prob=prob, sv=sv, sc=sc, uF=prob.fields(ownGrid=True), c0=np.array(sc['c']),
                                              rho0=np.array(sc['rho']) if density else None)
    return out


def test_own_grid_fields_and_their_data(solved):
    s = solved[('noninteger', 'fixed', True)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    subs = prob.system.subProblems
    assert [u.shape for u in uF] == [(int(op.nz) * int(op.nx), sv.nsrc) for op in subs]
    assert uF[0].shape[0] < prob.nrow and uF[1].shape[0] == prob.nrow
    assert np.array_equal(sv.dpred(u=uF), sv.dpred())                            # sampled where they were solved: no round trip through the native grid
    assert [u.shape for u in prob.fields()] == [(prob.nrow, sv.nsrc)] * 2        # (the default stays the up-scaled fields)
    adj = prob.adjointSystem
    assert [(op.nz, op.nx) for op in adj.subProblems] == [(op.nz, op.nx) for op in subs] and all(op.transposed for op in adj.subProblems)


def _taylor(s, what):
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    shape = (sv.nrec, sv.nsrc, sv.nfreq)
    N = prob.nrow
    vc, vr = mc.everywhere(21), mc.everywhere(22)
    try:
        if what == 'c':
            Jv = prob.JvecBorn(None, vc, u=uF, **FULL)
            return mc.per_frequency_factors(lambda c: sv.dpred(c), Jv, s['c0'], vc, shape)
        if what == 'rho':
            Jv = prob.JvecBorn(None, vr, u=uF, parameter='rho', **FULL)
            return mc.per_frequency_factors(lambda rho: sv.dpred({'rho': np.array(rho)}), Jv, s['rho0'], vr, shape)
        Jv = prob.JvecBorn(None, np.concatenate((vc, vr)), u=uF, parameter='joint', **FULL)
        return mc.per_frequency_factors(lambda x: sv.dpred({'c': np.array(x[0]), 'rho': np.array(x[1])}), Jv, (s['c0'], s['rho0']),
                                        (vc.reshape((mc.NZ, mc.NX)), vr.reshape((mc.NZ, mc.NX))), shape)
    finally:
        prob.updateModel({'c': np.array(s['c0'])} if s['rho0'] is None else {'c': np.array(s['c0']), 'rho': np.array(s['rho0'])})
        assert N == prob.nrow


@pytest.mark.parametrize('what,density', [('c', True), ('c', False), ('rho', True), ('joint', True)], ids=['full-rho', 'full-gardner', 'rho', 'joint'])
@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_taylor_remainder_of_dpred_falls_at_second_order_on_every_grid(solved, key, what, density):
    'a perturbation that is non-zero in every native cell, five halvings, every factor of every frequency in the second-order window'
    f = _taylor(solved[key + (density,)], what)
    print('%s %s %s: factors per frequency %s' % (key, what, 'rho' if density else 'gardner', np.round(f.T, 3).tolist()))
    assert f.shape == (5, 2) and np.all(f >= mc.SECOND)


@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_operator_is_exact_where_the_perturbation_vanishes_in_the_layers_of_every_grid(solved, key):
    s = solved[key + (True,)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    v = mc.layer_free(sv)
    Jop = prob.JvecBorn(None, v, u=uF, **OP)
    assert ac.rel(Jop, prob.JvecBorn(None, v, u=uF, **FULL)) <= 1e-10
    try:
        f = mc.per_frequency_factors(lambda c: sv.dpred(c), Jop, s['c0'], v, (sv.nrec, sv.nsrc, sv.nfreq))
    finally:
        prob.updateModel(np.array(s['c0']))
    print('%s operator: factors per frequency %s' % (key, np.round(f.T, 3).tolist()))
    assert np.all(f >= mc.SECOND)
    # on a perturbation that is non-zero in the layers 'operator' is of first order: the gap 'full' closes
    ve = mc.everywhere(21)
    try:
        fe = mc.per_frequency_factors(lambda c: sv.dpred(c), prob.JvecBorn(None, ve, u=uF, **OP), s['c0'], ve, (sv.nrec, sv.nsrc, sv.nfreq))
    finally:
        prob.updateModel(np.array(s['c0']))
    assert np.all(fe[-1] <= 2.5)


SERVED = [('operator', 'c'), ('operator', 'rho'), ('operator', 'joint'), ('full', 'c'), ('full', 'rho'), ('full', 'joint')]


@pytest.mark.parametrize('hd', [False, True], ids=['mz', 'hd'])
@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_every_served_pair_is_adjoint_and_the_upscaler_is_not(helm_lib, key, hd):
    prob, sv, sc = mc.host_pair(*key, hd=hd, **(dict(scaleTerm=0.7 - 0.2j) if hd else {}))
    uF = prob.fields(ownGrid=True)
    rng = np.random.default_rng(17)
    N = prob.nrow
    # one frequency's residual at a time: each frequency lives on a grid of its own, and in a sum the one with the largest data would hide the others
    R = ac.randc(rng, (sv.nrec, sv.nsrc, sv.nfreq))
    rs = []
    for i in range(sv.nfreq):
        ri = np.zeros_like(R)
        ri[:, :, i] = R[:, :, i]
        rs.append(ri.ravel())
    exact = {}
    for lin, par in SERVED:
        x = rng.standard_normal(2 * N if par == 'joint' else N)
        Jx = prob.JvecBorn(None, x, u=uF, linearisation=lin, parameter=par)
        assert Jx.shape == (sv.nD,) and Jx.dtype == np.complex128
        for i, r in enumerate(rs):
            g = prob.Jtvec(None, r, u=uF, adjoint='transpose', linearisation=lin, parameter=par)
            assert g.dtype == np.float64 and g.shape == x.shape
            lhs = ac.inner(Jx, r)
            exact[(lin, par, i)] = (x, lhs)
            miss = abs(lhs - ac.inner(x, g)) / abs(lhs)
            print('%s %s %s %s frequency %d: identity misses by %.2e' % (key, 'hd' if hd else 'mz', lin, par, i, miss))
            assert miss <= 1e-10
    # u = None solves the per-grid fields itself
    r = R.ravel()
    assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', **FULL), prob.Jtvec(None, r, u=uF, adjoint='transpose', **FULL)) <= 1e-12
    assert ac.rel(prob.JvecBorn(None, x[:N], **FULL), prob.JvecBorn(None, x[:N], u=uF, **FULL)) <= 1e-12
    # negative control on the coarse frequency: the interpolation back up in the place of the transpose
    assert sv.mgHelper.scales[0] > 1.
    for ds in set(sv.preProcessors):
        ds._adjoint = ds.T
    x, lhs = exact[('full', 'c', 0)]
    wrong = abs(lhs - ac.inner(x, prob.Jtvec(None, rs[0], u=uF, adjoint='transpose', **FULL))) / abs(lhs)
    print('%s: with ds.T for the adjoint the identity misses by %.2e' % (key, wrong))
    assert wrong > 1e-6


@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_hvec_is_the_composition_and_the_joint_halves_are_the_single_calls(solved, key):
    s = solved[key + (True,)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    N = prob.nrow
    rng = np.random.default_rng(23)
    x, y = rng.standard_normal(N), rng.standard_normal(N)
    wts = rng.uniform(0., 2., sv.nD)
    H = prob.Hvec(None, x, u=uF, weights=wts, **FULL)
    ref = prob.Jtvec(None, prob.JvecBorn(None, x, u=uF, **FULL) * wts, u=uF, adjoint='transpose', **FULL)
    assert ac.rel(H, ref) <= 1e-12
    a, b = float(y @ prob.Hvec(None, x, u=uF, **FULL)), float(x @ prob.Hvec(None, y, u=uF, **FULL))
    print('%s: symmetry defect of Hvec %.2e' % (key, abs(a - b) / max(abs(a), abs(b))))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    Hc = prob.Hvec(None, x, u=uF, parameter=('c', 'rho'), **FULL)
    assert ac.rel(Hc, prob.Jtvec(None, prob.JvecBorn(None, x, u=uF, **FULL), u=uF, adjoint='transpose', parameter='rho', **FULL)) <= 1e-12
    r = ac.randc(rng, sv.nD)
    for lin in (FULL, OP):
        gj = prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter='joint', **lin)
        assert ac.rel(gj[:N], prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter='c', **lin)) <= 1e-12
        assert ac.rel(gj[N:], prob.Jtvec(None, r, u=uF, adjoint='transpose', parameter='rho', **lin)) <= 1e-12
        dj = prob.JvecBorn(None, np.concatenate((x, y)), u=uF, parameter='joint', **lin)
        assert ac.rel(dj, prob.JvecBorn(None, x, u=uF, parameter='c', **lin) + prob.JvecBorn(None, y, u=uF, parameter='rho', **lin)) <= 1e-12
    Hj = prob.Hvec(None, np.concatenate((x, y)), u=uF, parameter='joint', **FULL)
    assert Hj.shape == (2 * N,)


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
def test_scales_all_one_give_the_single_grid_results(helm_lib, mode, density):
    from zephyr_amd.distributors import MultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    prob, sv, sc = mc.host_pair('noninteger', mode, density=density, freqs=[25., 30.])
    assert sv.mgHelper.scales == [1., 1.]
    one = dict(sc, SystemWrapper=MultiFreq)
    for k in ('cMin', 'targetGPW', 'multiscaleDerivatives', 'hostTransfer'):
        one.pop(k)
    p1, s1 = Helm2DProblem(one), Helm2DSurvey(one)
    p1.pair(s1)
    rng = np.random.default_rng(4)
    N = prob.nrow
    r = ac.randc(rng, sv.nD)
    for lin, par in (SERVED if density else [('full', 'c')]):
        x = rng.standard_normal(2 * N if par == 'joint' else N)
        kw = dict(linearisation=lin, parameter=par)
        assert ac.rel(prob.JvecBorn(None, x, **kw), p1.JvecBorn(None, x, **kw)) <= 1e-12
        assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', **kw), p1.Jtvec(None, r, adjoint='transpose', **kw)) <= 1e-12
        assert ac.rel(prob.Hvec(None, x, **kw), p1.Hvec(None, x, **kw)) <= 1e-12


def test_host_lists_must_be_per_grid(solved):
    s = solved[('noninteger', 'fixed', True)]
    prob, sv = s['prob'], s['sv']
    native = prob.fields()
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for call in (lambda: prob.Jtvec(None, r, u=native, adjoint='transpose', **FULL), lambda: prob.JvecBorn(None, v, u=native, **FULL),
                 lambda: prob.Hvec(None, v, u=native, **FULL)):
        with pytest.raises(ValueError, match='ownGrid=True'):
            call()


def _refused(call, *words):
    with pytest.raises(NotImplementedError) as ei:
        call()
    msg = str(ei.value)
    assert len(msg) > 20 and all(w in msg for w in words), msg
    return msg


def test_what_the_key_does_not_serve_is_refused_with_a_sentence_of_its_own(solved):
    import zephyr_amd as za
    from zephyr_amd.interpolation import BaseGridInterpolator
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoMultiGridProblem, Helm25DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey, Helm25DMultiGridSurvey
    s = solved[('noninteger', 'fixed', True)]
    prob, sv = s['prob'], s['sv']
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    seen = set()
    for call in (lambda: prob.Jtvec(None, r, adjoint='transpose'), lambda: prob.JvecBorn(None, v), lambda: prob.Hvec(None, v)):
        seen.add(_refused(call, "'scaler'", 'multiscale').split(' with ')[1])
    seen.add(_refused(lambda: prob.Hvec(None, v, resid=r, **FULL), 'Hvec(resid=)', 'multiscale'))
    for kw in (dict(kind='gaussNewton'), dict(kind='pseudoHessian', linearisation='full'), dict(kind='pseudoHessian', linearisation='operator', parameter='rho'),
               dict(kind='gaussNewton', linearisation='full')):
        seen.add(_refused(lambda: prob.illumination(**kw), 'illumination', 'diag(S^T H S)'))
    seen.add(_refused(lambda: prob.hessianBlocks(), 'hessianBlocks', 'diag(S^T H S)'))
    with pytest.raises(RuntimeError, match='device path'):          # (hostGradient: no store, as on a single grid)
        prob.fieldsDevice()
    # the other multiscale pairings
    scv = mc.problem_config(Disc=ac.OracleMiniZephyrT, hostGradient=True, hostTransfer=True, Q=50., viscoDerivatives=True, SystemWrapper=za.ViscoMultiGridMultiFreq)
    sc25 = mc.problem_config(Disc=ac.OracleMiniZephyr25DT, hostGradient=True, hostTransfer=True, nky=2, kyOnDevice=False, kyDerivatives=True, cmin=1500.)
    sce = mc.problem_config(Disc=za.Eurus, hostGradient=True, hostTransfer=True, eurusDerivatives=True)

    class NoAdjoint(BaseGridInterpolator):
        pass
    scn = mc.problem_config(Disc=ac.OracleMiniZephyrT, hostGradient=True, GridInterpolator=NoAdjoint)
    for P, S, sc, word in ((Helm2DViscoMultiGridProblem, Helm2DMultiGridSurvey, scv, 'visco'), (Helm25DProblem, Helm25DMultiGridSurvey, sc25, '2.5-D'),
                           (Helm2DProblem, Helm2DMultiGridSurvey, sce, 'Eurus'), (Helm2DProblem, Helm2DMultiGridSurvey, scn, '.adjoint')):
        p, q = P(sc), S(sc)
        p.pair(q)
        rr, vv = np.ones(q.nD, dtype=complex), np.ones(p.nrow)
        for call in (lambda: p.Jtvec(None, rr, adjoint='transpose', **FULL), lambda: p.JvecBorn(None, vv, **FULL), lambda: p.Hvec(None, vv, **FULL)):
            seen.add(_refused(call, 'multiscaleDerivatives', word).split(' with ', 1)[1])
    assert len(seen) >= 8                                  # a sentence of its own each: scaler, resid, diagonals, blocks, and the four pairings
    # what stays as it was, either way
    g = prob.Jtvec(None, r)
    assert g.shape == (prob.nrow,) and np.iscomplexobj(g)
    assert prob.illumination(kind='energy').shape == (prob.nrow,) and prob.illumination(kind='pseudoHessian').shape == (prob.nrow,)
    assert prob.Jvec(None, v).shape == (sv.nD,)


def test_without_the_key_every_refusal_is_what_it_was(helm_lib):
    sentence = 'serves single-grid surveys: the transposed operator and the stored forward fields live on one grid'
    prob, sv, sc = mc.host_pair(multiscaleDerivatives=False)
    prob2, sv2, _ = mc.host_pair()
    sc.pop('multiscaleDerivatives')
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    prob3, sv3 = Helm2DProblem(sc), Helm2DMultiGridSurvey(sc)
    prob3.pair(sv3)
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for p in (prob, prob3):
        for lin in ('scaler', 'operator', 'full'):
            kw = dict(linearisation=lin)
            for what, call in (("Jtvec(adjoint='transpose')", lambda: p.Jtvec(None, r, adjoint='transpose', **kw)), ('JvecBorn', lambda: p.JvecBorn(None, v, **kw)),
                               ('Hvec', lambda: p.Hvec(None, v, **kw))):
                msg = _refused(call, sentence)
                assert msg.startswith(what)
        _refused(lambda: p.adjointSystem, 'the transposed operator serves single-grid problems: a multiscale pairing has no exact-adjoint route')
        _refused(lambda: p.fieldsDevice(), 'fieldsDevice serves single-grid surveys: on a multiscale survey the u-given branch of Jtvec multiplies the native-grid forward')
        _refused(lambda: p.illumination(kind='gaussNewton'), sentence)
        _refused(lambda: p.illumination(linearisation='full'), sentence)
        _refused(lambda: p.hessianBlocks(), sentence)
        # the mux gradient and the data are what the pairing with the key gives too
        assert np.array_equal(p.Jtvec(None, r), prob2.Jtvec(None, r)) and np.array_equal(p.survey.dpred(), sv2.dpred())


WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests import multiscale_exact_cases as mc
ref, sref, _ = mc.host_pair('noninteger', 'relative', shardFreqs=False)
prob, sv, _ = mc.host_pair('noninteger', 'relative')
assert prob.ownedFreqs == [dist.get_rank()] and ref.ownedFreqs == [0, 1]
rng = np.random.default_rng(5)
v, r = rng.standard_normal(2 * prob.nrow), ac.randc(rng, sv.nD)
kw = dict(linearisation='full', parameter='joint')
ok = ac.rel(prob.Jtvec(None, r, adjoint='transpose', **kw), ref.Jtvec(None, r, adjoint='transpose', **kw)) < 1e-12
ok = ok and ac.rel(prob.JvecBorn(None, v, **kw), ref.JvecBorn(None, v, **kw)) < 1e-12
ok = ok and ac.rel(prob.Hvec(None, v, **kw), ref.Hvec(None, v, **kw)) < 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(tmp_path):
    'the two frequencies -- two grids -- sharded over two ranks: the all-reduce is of the native-grid vector, and every rank holds the single-rank result'
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29657', WORLD_SIZE='2', PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o


def test_untouched_nodes_read_where_their_neighbours_read(helm_lib):
    """at an integer scale s all but every s-th native node is touched by no output: its all-zero window starts where its nearest touched neighbour's does, so
    that a tile of 256 native columns spans about 256 / s + WT coarse elements and not the whole row up to its right edge"""
    from zephyr_amd.interpolation import regrid_axis_t
    for n_in, n_out, h in ((1024, 256, 4.), (30, 8, 4.), (1024, 468, 1024 / 468.)):
        M, _ = dense_axis(n_in, 1., n_out, h)
        start, taps = regrid_axis_t(n_in, 1., n_out, h)
        WT = taps.shape[1]
        touched = M.any(axis=0)
        near = None
        for j in range(n_in):
            if touched[j]:
                near = start[j]
            elif near is not None:
                assert start[j] == near and not taps[j].any()
        first = int(np.argmax(touched))
        assert np.all(start[:first] == start[first])
        for c0 in range(0, n_in, 256):
            span = int((start[c0:c0 + 256] + WT).max() - start[c0:c0 + 256].min())
            assert span <= 256 / h + WT + 1, (n_in, h, c0, span)


def test_up_sampling_is_refused_on_the_host_route_too(helm_lib):
    up = interpolator((101, 101), 3., hostTransfer=True).T
    with pytest.raises(NotImplementedError, match='more than 64'):
        up.adjoint * np.zeros(up.shape[0])


def test_adjoint_system_says_why_a_pairing_is_not_served(helm_lib):
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DViscoMultiGridProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    scv = mc.problem_config(Disc=ac.OracleMiniZephyrT, hostGradient=True, hostTransfer=True, Q=50., viscoDerivatives=True, SystemWrapper=za.ViscoMultiGridMultiFreq)
    p, q = Helm2DViscoMultiGridProblem(scv), Helm2DMultiGridSurvey(scv)
    p.pair(q)
    _refused(lambda: p.adjointSystem, 'adjointSystem', 'multiscaleDerivatives', 'visco')
