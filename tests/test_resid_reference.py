"""CPU: the reference and the bounds of tests/test_gpu_resid_stage.py (tests/resid_cases.py) checked without a GPU -- the extended-precision stencil agrees
with the oracle's sparse matrix, a plain complex128 evaluation of q' - A x satisfies every bound (so a failure on the GPU means the kernel, not the bound),
and the test hook helm_debug_nm_stage refuses malformed input before it touches a device."""
import numpy as np
import pytest

from oracle import helm_oracle as ho
from tests import resid_cases as rc


@pytest.fixture
def x87():
    if not rc.have_x87():
        pytest.skip('numpy.longdouble is not the 80-bit x87 format on this host: no extended-precision reference')


@pytest.mark.parametrize('kind,nz,nx', [('mz', 9, 70), ('eurus', 33, 65), ('random', 5, 33)])
def test_extended_reference_agrees_with_the_oracle_matrix(x87, kind, nz, nx):
    C, x, q = rc.operands(kind, nz, nx, 7, 'random')
    ref = rc.Ref(C, x, q)
    want = q - ho.coefficients_to_csr(C) @ x
    err = np.linalg.norm(ref.r.astype(np.complex128) - want) / np.linalg.norm(want)
    print('%s %d x %d: reference against csr @ x, relative %.2e' % (kind, nz, nx, err))
    assert err <= 1e-13
    assert np.allclose(ho.stencil_apply(C, x), ho.coefficients_to_csr(C) @ x, rtol=0, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize('kind,nz,nx,ncol', [('mz', 9, 70, 5), ('eurus', 33, 65, 3), ('random', 5, 33, 9), ('random', 1, 1, 2), ('random', 2, 200, 3)])
@pytest.mark.parametrize('regime', ['random', 'cancel'])
def test_a_plain_fp64_evaluation_satisfies_every_bound(x87, kind, nz, nx, ncol, regime):
    C, x, q = rc.operands(kind, nz, nx, ncol, regime)
    rng = np.random.default_rng(3)
    keep = rng.random(x.shape) < 0.6
    worst = {}
    for osc in rc.OSCALES:
        for xin_is_u in (False, True):
            for qkeep in (None, keep):
                xin = np.conj(osc * x) if xin_is_u else x
                ref = rc.Ref(C, xin, q, oscale=osc, xin_is_u=xin_is_u, qkeep=qkeep)
                for order, seq in ((range(9), False), (range(8, -1, -1), True)):
                    r, rr, qq, u = rc.resid_fp64(C, xin, q, oscale=osc, xin_is_u=xin_is_u, qkeep=qkeep, order=order, sequential=seq)
                    got = dict(stored=rc.ratio_stored(r, ref), uout=rc.ratio_uout(u, ref, osc), rr_stored=rc.ratio_rr_stored(rr, r),
                               rr_norms=rc.ratio_rr_norms(rr, ref), qq=rc.ratio_qq(qq, ref))
                    for k, v in got.items():
                        worst[k] = max(worst.get(k, 0.0), v)
    print('%s %d x %d x %d %s: worst ratios %s' % (kind, nz, nx, ncol, regime, {k: round(v, 4) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_prep_bound_admits_a_plain_fp64_evaluation(x87):
    rng = np.random.default_rng(5)
    rhs, sub = rc.crand(rng, 7, 100), rc.crand(rng, 7, 100)
    for premul in (1 + 0j, 0.5 - 2j):
        for s in (None, sub):
            Qt = (premul * rhs - (0 if s is None else s)).T
            assert rc.ratio_prep(Qt, rhs, premul, s) <= 1.0
    assert rc.ratio_prep((rhs * (1 + 1e-15)).T, rhs, 1 + 0j, None) == np.inf          # premul = 1 without sub: the same bits


def test_a_wrong_residual_does_not_pass(x87):
    """the checks have teeth: one dropped tap, one column off, or a norm short of one cell is outside the bounds"""
    for regime in ('random', 'cancel'):
        C, x, q = rc.operands('mz', 9, 70, 5, regime)
        ref = rc.Ref(C, x, q)
        r, rr, qq, _ = rc.resid_fp64(C, x, q)
        dropped, _, _, _ = rc.resid_fp64(C, x, q, order=range(8))
        assert rc.ratio_stored(dropped, ref) > 1e6
        assert rc.ratio_stored(np.roll(r, 1, axis=1), ref) > (1e6 if regime == 'random' else 1.0)     # (cancel: the neighbour's residual is rounding too)
        cell = np.argmax(np.abs(r[:, 0]))
        short = rr.copy()
        short[0] -= abs(r[cell, 0]) ** 2
        assert rc.ratio_rr_stored(short, r) > 1e3
        assert regime == 'cancel' or rc.ratio_rr_norms(short, ref) > 1.0             # (cancel: ||r|| is below its own bound, only the stored form can tell)
        assert rc.ratio_qq(qq * (1 + 1e-10), ref) > 1.0


def resid_args(nz=5, nx=7, ncol=9, pad=2):
    N = nz * nx
    ld = ncol + pad
    z = lambda n: np.zeros(n, complex)
    return dict(nz=nz, nx=nx, ncol=ncol, planes=z(9 * N), Xin=z(N * ld), ldin=ld, Q=z(N * ld), ldq=ld, nblk_cap=0)


def test_nm_stage_refuses_malformed_input_before_it_touches_a_device(helm_lib):
    """Every case is refused with HELM_ERR_ARG by the host-side check that runs before hipSetDevice: the answer is the same with and without a GPU (a
    well-formed call answers HELM_ERR_DEVICE on a host without one)."""
    ARG = rc.HELM_ERR_ARG
    call = lambda stage, **a: rc.nm_stage(helm_lib, stage, **a)[0]
    ok = resid_args()
    assert call(rc.RESID, **ok) != ARG
    N = 35
    # negative or zero sizes, an unknown stage
    for k in ('nz', 'nx', 'ncol'):
        for v in (0, -3):
            assert call(rc.RESID, **dict(ok, **{k: v})) == ARG, (k, v)
    assert call(rc.RESID, **dict(ok, nblk_cap=-1)) == ARG
    assert call(7, **ok) == ARG and call(-1, **ok) == ARG
    # leading dimensions smaller than the width; buffers shorter than the leading dimension says
    for k in ('ldin', 'ldq'):
        for v in (8, 0, -11):
            assert call(rc.RESID, **dict(ok, **{k: v})) == ARG, (k, v)
    assert call(rc.RESID, **dict(ok, ldq=-11, qmap=np.zeros(9, np.int32))) == ARG
    for k, ln in (('Xin', 'xin_len'), ('Q', 'q_len'), ('planes', 'planes_len')):
        assert call(rc.RESID, **dict(ok, **{ln: ok[k].size - 3})) == ARG, k
        assert call(rc.RESID, **dict(ok, **{k: None})) == ARG, k
    out = np.zeros(N * 11, complex)
    assert call(rc.RESID, **dict(ok, store=1, Rout=out)) != ARG
    assert call(rc.RESID, **dict(ok, store=1, Rout=out, rout_len=out.size - 3)) == ARG
    assert call(rc.RESID, **dict(ok, store=0, Rout=out)) == ARG                               # an output nobody writes
    assert call(rc.RESID, **dict(ok, store=2)) == ARG
    assert call(rc.RESID, **dict(ok, Uout=out, ldu=11)) != ARG
    assert call(rc.RESID, **dict(ok, Uout=out, ldu=8)) == ARG
    assert call(rc.RESID, **dict(ok, Uout=out, ldu=12)) == ARG
    assert call(rc.RESID, **dict(ok, no_rr=True)) == ARG and call(rc.RESID, **dict(ok, qnorm=1, no_qq=True)) == ARG
    # the column map: an entry at or beyond ldq, a negative one, a repeated one when r is stored, a mask beside it
    qmap = np.arange(9, dtype=np.int32)[::-1].copy()
    assert call(rc.RESID, **dict(ok, qmap=qmap)) != ARG
    for j, v in ((4, 11), (0, -1)):
        bad = qmap.copy()
        bad[j] = v
        assert call(rc.RESID, **dict(ok, qmap=bad)) == ARG, (j, v)
    rep = qmap.copy()
    rep[3] = rep[5]
    assert call(rc.RESID, **dict(ok, qmap=rep)) != ARG and call(rc.RESID, **dict(ok, qmap=rep, store=1)) == ARG
    mask = np.zeros(N, np.uint8)
    assert call(rc.RESID, **dict(ok, qmask=mask)) != ARG
    assert call(rc.RESID, **dict(ok, qmask=mask, qmap=qmap)) == ARG
    # the other stages
    z = lambda n: np.zeros(n, complex)
    prep = dict(N=20, ncol=3, Xin=z(3 * 30), rhs_ld=30, row_off=5, Rout=z(60), Q=z(60))
    assert call(rc.PREP, **prep) != ARG
    for bad in (dict(rhs_ld=24), dict(row_off=-1), dict(row_off=11), dict(xin_len=84), dict(rout_len=59), dict(q_len=59), dict(N=0), dict(N=-2), dict(Rout=None),
                dict(no_qq=True)):
        assert call(rc.PREP, **dict(prep, **bad)) == ARG, bad
    cols = np.array([4, 0, 2], np.int32)
    pack = dict(N=20, ncol=3, Xin=z(20 * 6), ldin=6, qmap=cols, Rout=z(60))
    assert call(rc.PACK, **pack) != ARG
    for bad in (dict(qmap=np.array([4, 6, 2], np.int32)), dict(qmap=None), dict(xin_len=20 * 6 - 2), dict(rout_len=59), dict(ldin=4)):
        assert call(rc.PACK, **dict(pack, **bad)) == ARG, bad
    scat = dict(N=20, ncol=3, Xin=z(60), Q=z(20 * 6), ldq=6, qmap=cols)
    assert call(rc.SCATTER_ADD, **scat) != ARG
    for bad in (dict(qmap=np.array([4, 4, 2], np.int32)), dict(q_len=20 * 6 - 2), dict(xin_len=59), dict(Q=None), dict(ldq=4)):
        assert call(rc.SCATTER_ADD, **dict(scat, **bad)) == ARG, bad
    for stage in (rc.RECOVER_X, rc.TRANSPOSE_OUT, rc.TRANSPOSE):
        a = dict(N=20, ncol=3, Xin=z(60), Rout=z(60))
        assert call(stage, **a) != ARG
        for bad in (dict(xin_len=59), dict(rout_len=59), dict(Xin=None), dict(conj=2)):
            assert call(stage, **dict(a, **bad)) == ARG, (stage, bad)
    assert call(rc.RECOVER_X, N=20, ncol=3, Xin=z(60), Rout=z(60), oscale=0j) == ARG
