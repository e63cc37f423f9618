"""GPU: the 2.5-D ky sum kept in HBM -- helm_axpby_device / helm_sample_accumulate_device against numpy within bounds derived from the number format,
MiniZephyr25D as a device operator (`*`, dpred, Jtvec) against the host reduction (kyOnDevice=False) and the goldens g8 / g11, transfers counted,
kyRelease, and the composite through the worker pipeline of MultiFreq."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -52                      # = 2u
ST = np.exp(1j * np.pi) / (4 * np.pi)
COEFFS = [(1.0 + 0j, 0j), (1.0 + 0j, 1.0 + 0j), (0.3 - 0.7j, 1.0 + 0j), (ST, ST)]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b))


def small_op():
    import zephyr_amd as za
    return za.MiniZephyr(dict(nx=20, nz=24, dx=10., dz=10., c=2500., freq=5., nPML=4))


def randc(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def axpby(lib, op, alpha, d_x, beta, d_y, n):
    from zephyr_amd import _lib
    _lib.check(lib.helm_axpby_device(op.handle, alpha.real, alpha.imag, ctypes.c_void_p(d_x), beta.real, beta.imag, ctypes.c_void_p(d_y), n), op.handle)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 2 ** 20 + 3, 64 * 512 * 512])
def test_axpby_against_numpy_within_the_format_bound(helm_lib, n):
    """|y - y_ref| <= 4 eps (|alpha||x| + |beta||y0|) for EVERY element: a complex product is within sqrt(5) u of the exact one in modulus, the sum adds u,
    (sqrt(5) + 1) u < 3.3 u for the kernel and the same again for numpy's value: 6.5 u < 8 u = 4 eps.  beta = 0: the accumulator holds NaN and is not read."""
    import torch
    op = small_op()
    dev = torch.device('cuda', op.device)
    rng = np.random.default_rng(1000 + n % 997)
    x, y0 = randc(rng, n), randc(rng, n)
    dx = torch.from_numpy(x).to(dev)
    for alpha, beta in COEFFS:
        if beta == 0:
            dy = torch.full((n,), float('nan'), dtype=torch.complex128, device=dev)
            ref, mag = alpha * x, abs(alpha) * np.abs(x)
        else:
            dy = torch.from_numpy(y0).to(dev)
            ref, mag = beta * y0 + alpha * x, abs(alpha) * np.abs(x) + abs(beta) * np.abs(y0)
        torch.cuda.synchronize(dev)
        axpby(helm_lib, op, alpha, dx.data_ptr(), beta, dy.data_ptr(), n)
        y = dy.cpu().numpy()
        assert np.isfinite(y.view(np.float64)).all(), (alpha, beta)
        err = np.abs(y - ref)
        worst = float((err / mag).max())
        print('axpby n=%d alpha=%s beta=%s: worst |err| / (|a||x| + |b||y0|) = %.3f eps' % (n, alpha, beta, worst / EPS))
        assert (err <= 4 * EPS * mag).all(), (n, alpha, beta, worst / EPS)
        assert np.array_equal(dx.cpu().numpy(), x)                 # X is read-only
    del op.factors


def test_axpby_on_sub_ranges_leaves_both_sides_untouched(helm_lib):
    import torch
    op = small_op()
    dev = torch.device('cuda', op.device)
    rng = np.random.default_rng(77)
    total = 9000
    x, y0 = randc(rng, total), randc(rng, total)
    for off, n in [(3, 255), (17, 1021), (1, 4099), (5, 1), (31, 8192), (2049, 2048 * 3 + 7)]:
        assert off % 16 != 0 and off + n < total
        for alpha, beta in COEFFS:
            dx, dy = torch.from_numpy(x).to(dev), torch.from_numpy(y0).to(dev)
            torch.cuda.synchronize(dev)
            axpby(helm_lib, op, alpha, dx.data_ptr() + 16 * (off + 2), beta, dy.data_ptr() + 16 * off, n)      # (X at another offset than Y)
            y = dy.cpu().numpy()
            assert np.array_equal(y[:off], y0[:off]) and np.array_equal(y[off + n:], y0[off + n:]), (off, n, alpha, beta)
            xs, ys = x[off + 2:off + 2 + n], y0[off:off + n]
            ref = alpha * xs + (beta * ys if beta != 0 else 0)
            mag = abs(alpha) * np.abs(xs) + abs(beta) * np.abs(ys)
            assert (np.abs(y[off:off + n] - ref) <= 4 * EPS * mag).all(), (off, n, alpha, beta)
    del op.factors


def g11_config(**kw):
    import zephyr_amd as za
    g = np.load(os.path.join(GOLD, 'g11_25d_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=za.MiniZephyr25D, nky=int(g['nky']), parallel=False,
              sterms=g['sterms'], geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), rtol=1e-11)
    sc.update(kw)
    return g, sc


def g11_pair(**kw):
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    g, sc = g11_config(**kw)
    prob, surv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(surv)
    return g, sc, prob, surv


def receiver_matrices():
    'the CSR receiver matrices of two real surveys: the g11 geometry, and a line of 128 receivers on the 512^2 grid'
    from zephyr_amd.survey import Helm25DSurvey, Helm2DSurvey
    _, sc = g11_config()
    out = [('g11', sp.csr_matrix(Helm25DSurvey(sc).rVec(0, 0)))]
    n, dx = 512, 10.
    rec = np.stack([np.linspace(100.0, dx * n - 100.0, 128), np.full(128, 20.0)], axis=1)
    src = np.array([[200., 20.]])
    sc2 = dict(nx=n, nz=n, dx=dx, dz=dx, c=2500., freqs=[4.], geom=dict(src=src, rec=rec, mode='fixed'))
    out.append(('line128_512', sp.csr_matrix(Helm2DSurvey(sc2).rVec(0, 0))))
    return out


def test_sample_accumulate_against_numpy_within_the_format_bound(helm_lib):
    """out = beta out + alpha R u per output within 2 (L + 4) 3.3 u (|alpha| sum_k |val_k||u_k| + |beta||out0|), L = entries of the CSR row: a complex dot
    product of L terms in any order, the product with alpha, the product with beta, the sum -- both sides' rounding."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    u = EPS / 2
    for name, Rm in receiver_matrices():
        Rm.sum_duplicates()
        nrec, N = Rm.shape
        assert nrec in (7, 128) and Rm.nnz > nrec
        nsrc = 5
        side = int(round(np.sqrt(N))) if name != 'g11' else None
        cfg = dict(nx=64, nz=48, dx=10., dz=10., c=2500., freq=5., nPML=6) if name == 'g11' else dict(nx=side, nz=side, dx=10., dz=10., c=2500., freq=4., nPML=10)
        op = za.MiniZephyr(cfg)
        assert op.nrow == N
        dev = torch.device('cuda', op.device)
        rng = np.random.default_rng(len(name))
        U = randc(rng, (nsrc, N))
        out0 = randc(rng, (nrec, nsrc))
        csr = (torch.from_numpy(Rm.indptr.astype(np.int64)).to(dev), torch.from_numpy(Rm.indices.astype(np.int64)).to(dev),
               torch.from_numpy(Rm.data.astype(np.complex128)).to(dev))
        dU = torch.from_numpy(U).to(dev)
        L = np.diff(Rm.indptr).reshape((nrec, 1))
        absdot = np.asarray(abs(Rm) @ np.abs(U.T))                     # sum_k |val_k||u_k| per (receiver, source)
        RU = np.asarray(Rm @ U.T)
        for alpha, beta in COEFFS:
            if beta == 0:
                dout = torch.full((nrec, nsrc), float('nan'), dtype=torch.complex128, device=dev)
                ref, mag = alpha * RU, abs(alpha) * absdot
            else:
                dout = torch.from_numpy(out0).to(dev)
                ref, mag = beta * out0 + alpha * RU, abs(alpha) * absdot + abs(beta) * np.abs(out0)
            torch.cuda.synchronize(dev)
            _lib.check(helm_lib.helm_sample_accumulate_device(op.handle, ctypes.c_void_p(dU.data_ptr()), nsrc, N, ctypes.c_void_p(csr[0].data_ptr()),
                                                              ctypes.c_void_p(csr[1].data_ptr()), ctypes.c_void_p(csr[2].data_ptr()), nrec,
                                                              alpha.real, alpha.imag, beta.real, beta.imag, ctypes.c_void_p(dout.data_ptr())), op.handle)
            out = dout.cpu().numpy()
            assert np.isfinite(out.view(np.float64)).all(), (name, alpha, beta)
            bound = 2 * (L + 4) * 3.3 * u * mag
            err = np.abs(out - ref)
            print('sample_accumulate %s alpha=%s beta=%s: worst err / bound = %.3f' % (name, alpha, beta, float((err / bound).max())))
            assert (err <= bound).all(), (name, alpha, beta, float((err / bound).max()))
        del op.factors


def test_g11_survey_device_ky_sum_against_golden_and_host_reduction(helm_lib):
    import zephyr_amd as za
    g, sc, prob, surv = g11_pair()
    _, sch, probh, survh = g11_pair(kyOnDevice=False)
    assert prob._deviceGradientAvailable() is True
    assert probh._deviceGradientAvailable() is False
    d = surv.dpred()
    assert rel(d, g['dpred']) <= 1e-7
    dh = survh.dpred()
    assert rel(d, dh) <= 1e-9
    rng = np.random.default_rng(5)
    resid = (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) * np.abs(d).mean()
    gd, gh = prob.Jtvec(None, resid), probh.Jtvec(None, resid)
    assert gd.shape == gh.shape == (prob.nrow,)
    assert rel(gd, gh) <= 1e-9
    # the composite's own product: sparse and dense right-hand sides, a vector included
    cfg = dict(sc, freq=float(g['freqs'][0]))
    opd, oph = za.MiniZephyr25D(cfg), za.MiniZephyr25D(dict(cfg, kyOnDevice=False))
    assert opd._onDevice() and not oph._onDevice()
    qs = surv.getSources()
    qs = qs[0] if isinstance(qs, (list, tuple)) else qs
    assert sp.issparse(qs)
    qd = np.asarray(qs.toarray()) * (1.0 + 0.5j) + 1e-3 * randc(np.random.default_rng(9), qs.shape)
    for q in (qs, qd, qd[:, 1].copy()):
        ud, uh = opd * q, oph * q
        assert ud.shape == uh.shape and ud.dtype == np.complex128
        assert rel(ud, uh) <= 1e-9
    assert rel((opd * qs)[:, 2], g['u_f0_src2']) <= 1e-7
    for o in (prob, probh, opd, oph):
        del o.factors
    assert not prob.factors and not opd.factors


def test_g8_reference_configuration_through_the_device_sum(helm_lib):
    import zephyr_amd as za
    g = np.load(os.path.join(GOLD, 'g8_25d.npz'))
    nx, nz = 100, 200
    sc = dict(c=2500., rho=1., nx=nx, nz=nz, freq=2e2, nky=20, parallel=False)
    op = za.MiniZephyr25D(sc)
    assert op._onDevice()
    u = (op * za.SimpleSource(sc)(np.array([[25., 25.]])))[:, 0].reshape((nz, nx))
    assert rel(u[np.arange(5, 196, 10), 60], g['line']) <= 1e-7
    assert op.factors and len(op.lastInfo) == 20
    del op.factors
    assert not any(sub.factors for sub in op.subProblems)
    sc4 = dict(sc, nky=4)
    u4 = (za.MiniZephyr25D(sc4) * za.SimpleSource(sc4)(np.array([[50., 100.]])))[:, 0].reshape((nz, nx))
    assert rel(u4[np.arange(5, 196, 10), 60], g['nky4_line']) <= 1e-7


def test_transfers_counted_one_download_for_the_device_sum(helm_lib, monkeypatch):
    """Around one `MiniZephyr25D * q` (N x 5, nky = 6): host-array solves (BaseDiscretization._solve: each brings its whole N x nsrc result back over PCIe)
    and downloads of at least N x 5 x 16 bytes through the Python-side helpers.  Device sum: 0 and 1.  Host reduction: nky and 0."""
    import zephyr_amd as za
    from zephyr_amd import _lib
    from zephyr_amd.discretization import BaseDiscretization
    g, sc = g11_config()
    cfg = dict(sc, freq=float(g['freqs'][0]), nky=6)
    N = cfg['nx'] * cfg['nz']
    q = za.SparseKaiserSource(cfg)(np.asarray(g['src'])[:5])
    assert q.shape == (N, 5)
    counts = dict(solve=0, down=0)
    real_solve, real_fd, real_fdp = BaseDiscretization._solve, _lib.from_device, _lib.from_device_pinned

    def solve(self, rhs, rows):
        counts['solve'] += 1
        return real_solve(self, rhs, rows)

    def counting(fn):
        def wrapped(t):
            if t.numel() * t.element_size() >= N * 5 * 16:
                counts['down'] += 1
            return fn(t)
        return wrapped
    monkeypatch.setattr(BaseDiscretization, '_solve', solve)
    monkeypatch.setattr(_lib, 'from_device', counting(real_fd))
    monkeypatch.setattr(_lib, 'from_device_pinned', counting(real_fdp))
    opd, oph = za.MiniZephyr25D(cfg), za.MiniZephyr25D(dict(cfg, kyOnDevice=False))
    ud = opd * q
    assert (counts['solve'], counts['down']) == (0, 1)
    counts.update(solve=0, down=0)
    uh = oph * q
    assert (counts['solve'], counts['down']) == (6, 0)
    assert rel(ud, uh) <= 1e-9
    del opd.factors, oph.factors


def test_ky_release_destroys_every_ky_operator_after_its_last_solve(helm_lib):
    g, sc, prob, surv = g11_pair(kyRelease=True)
    _, _, probr, survr = g11_pair()
    d = surv.dpred()
    comps = prob.system.subProblems
    assert len(comps) == len(g['freqs']) and all(len(c.subProblems) == int(g['nky']) for c in comps)
    assert not any(sub.factors for c in comps for sub in c.subProblems)
    assert not prob.factors
    dr = survr.dpred()
    assert any(sub.factors for c in probr.system.subProblems for sub in c.subProblems)       # (the default: resident until `del factors`)
    assert rel(d, dr) <= 1e-9
    d2 = surv.dpred()                                  # the handles are rebuilt
    assert rel(d2, dr) <= 1e-9
    assert not any(sub.factors for c in comps for sub in c.subProblems)
    rng = np.random.default_rng(5)
    resid = randc(rng, d.shape) * np.abs(d).mean()
    assert rel(prob.Jtvec(None, resid), probr.Jtvec(None, resid)) <= 1e-9
    assert not any(sub.factors for c in comps for sub in c.subProblems)
    del probr.factors


@pytest.mark.parametrize('nfreq', [1, 3])
def test_composite_through_the_worker_pipeline_of_multifreq(helm_lib, monkeypatch, nfreq):
    """`MultiFreq(Disc=MiniZephyr25D, parallel=True) * q` with two workers on GPU 0: one frequency -> its six sources are split and `_replica` builds a second
    composite; three frequencies -> no split."""
    import zephyr_amd as za
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    g, sc = g11_config(nky=3)
    freqs = [4., 6., 9.][:nfreq]
    locs = np.stack([np.linspace(120., 520., 6), np.linspace(90., 380., 6)], axis=1)
    q = za.SparseKaiserSource(dict(sc, freq=freqs[0]))(locs)
    par = za.MultiFreq(dict(sc, freqs=freqs, parallel=True))
    ser = za.MultiFreq(dict(sc, freqs=freqs, parallel=False))
    assert len(par.devices) == 2
    up, us = list(par * q), list(ser * q)
    assert len(up) == len(us) == nfreq
    for a, b in zip(up, us):
        assert a.shape == b.shape == (q.shape[0], 6)
        assert rel(a, b) <= 1e-9
    reps = par.__dict__.get('_replicas', {})
    if nfreq == 1:
        assert len(reps) == 1 and all(isinstance(r, za.MiniZephyr25D) and r._onDevice() for r in reps.values())
    else:
        assert not reps
    del par.factors, ser.factors
