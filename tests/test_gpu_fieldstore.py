"""GPU: forward wavefields kept in HBM between fieldsDevice(), dpred(u=F) and Jtvec(u=F) -- the three kernels of the complex64 store against numpy and
extended precision within bounds derived from the number formats, then the g6 survey (fixed and moving array), transfers and solves counted, source
batches on two workers, the 2.5-D composite, the complex64 store against the complex128 one, and what is refused."""
import ctypes
import os

import numpy as np
import pytest

from tests import test_gpu_moving as tm
from tests.fieldstore_cases import NCOL, pack_columns, pack_bound_violations

pytestmark = pytest.mark.gpu

GOLD = tm.GOLD
U_RND = 2.0 ** -53
rel, randc = tm.rel, tm.randc
P = ctypes.c_void_p


@pytest.fixture(scope='module')
def op(helm_lib):
    import zephyr_amd as za
    o = za.MiniZephyr(dict(nx=tm.NX, nz=tm.NZ, dx=10., dz=10., c=2500., freq=5., nPML=6))
    assert o.nrow == 4800 and o.nrow % 256 != 0 and o.handle
    yield o
    del o.factors


def wide_fields(rng, nsrc, N):
    'nsrc wavefields of N points whose magnitudes differ by sixteen decades between columns and by six within one'
    U = randc(rng, (N, nsrc)) * 10.0 ** rng.uniform(-8, 8, nsrc)[None, :]
    return U * 10.0 ** rng.uniform(-6, 0, (N, nsrc))


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [1, 4800])
@pytest.mark.parametrize('nsrc', [1, 5, 13])
def test_pack_kernel_exponents_exact_values_within_the_format_bound_guards_untouched(helm_lib, op, nsrc, ld):
    """helm_pack_c64_device on columns from 1e-300 to 1e300 (a zero column, a subnormal one, a maximum in the last element, an element 2^-140 of its
    column's maximum): the exponents are pack_reference's exactly, every component is within the bound of the format of the fp64 input, the guard regions
    around both outputs are untouched, and two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    dev = torch.device('cuda', op.device)
    Uall = pack_columns(ld)
    guard = 1031
    for start in range(0, NCOL - nsrc + 1, max(1, nsrc - 1)):
        U = Uall[:, start:start + nsrc]
        _, e_ref = pack_reference(U)
        dU = torch.from_numpy(np.ascontiguousarray(U.T)).to(dev)
        runs = []
        for _ in range(2):
            out = torch.full((2 * guard + nsrc * ld,), complex(7.0, -3.0), dtype=torch.complex64, device=dev)
            ex = torch.full((2 * guard + nsrc,), -77777, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            _lib.check(helm_lib.helm_pack_c64_device(op.handle, P(dU.data_ptr()), nsrc, ld, P(out.data_ptr() + 8 * guard), P(ex.data_ptr() + 4 * guard)), op.handle)
            h, he = out.cpu().numpy(), ex.cpu().numpy()
            assert np.all(h[:guard] == np.complex64(7.0 - 3.0j)) and np.all(h[guard + nsrc * ld:] == np.complex64(7.0 - 3.0j))
            assert np.all(he[:guard] == -77777) and np.all(he[guard + nsrc:] == -77777)
            runs.append((h[guard:guard + nsrc * ld].reshape((nsrc, ld)).T.copy(), he[guard:guard + nsrc].copy()))
        (Pk, e), (Pk2, e2) = runs
        assert np.array_equal(e, e_ref), (start, e, e_ref)
        assert np.array_equal(e, e2) and np.array_equal(Pk.view(np.uint32), Pk2.view(np.uint32))
        assert pack_bound_violations(U, unpack_reference(Pk, e), e) == 0, start
    assert dU.cpu().numpy().shape == (nsrc, ld)


@pytest.mark.parametrize('nsrc', [1, 5, 13])
def test_imaging_c64_kernel_against_extended_precision(helm_lib, op, nsrc):
    """helm_imaging_accumulate_c64_device against a longdouble evaluation of G0 + scaler sum_s u^F_s uB_s from the UNPACKED u^F, per point within
    2 (nsrc + 5) 3.3 u (|scaler| sum_s |u^F_s||uB_s| + |G0|), u = 2^-53: the rescaling is exact, so this is k_imaging's sum with its term count."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    dev = torch.device('cuda', op.device)
    N = op.nrow
    rng = np.random.default_rng(40 + nsrc)
    Pk, e = pack_reference(wide_fields(rng, nsrc, N))
    UFh = unpack_reference(Pk, e)
    UB = wide_fields(rng, nsrc, N)
    scaler, G0 = randc(rng, N) * 1e-3, randc(rng, N) * np.abs(UFh * UB).sum(axis=1).mean() * 1e-3
    dP, dE = torch.from_numpy(np.ascontiguousarray(Pk.T)).to(dev), torch.from_numpy(e).to(dev)
    dB, dS = torch.from_numpy(np.ascontiguousarray(UB.T)).to(dev), torch.from_numpy(scaler).to(dev)
    outs = []
    for _ in range(2):
        dG = torch.from_numpy(G0).to(dev)
        torch.cuda.synchronize(dev)
        _lib.check(helm_lib.helm_imaging_accumulate_c64_device(op.handle, P(dP.data_ptr()), P(dE.data_ptr()), P(dB.data_ptr()), nsrc, P(dS.data_ptr()), P(dG.data_ptr())), op.handle)
        outs.append(dG.cpu().numpy())
    assert np.array_equal(outs[0].view(np.float64), outs[1].view(np.float64))
    cl = np.clongdouble
    ref = G0.astype(cl) + scaler.astype(cl) * (UFh.astype(cl) * UB.astype(cl)).sum(axis=1)
    bound = 2 * (nsrc + 5) * 3.3 * U_RND * (np.abs(scaler) * (np.abs(UFh) * np.abs(UB)).sum(axis=1) + np.abs(G0))
    err = np.abs(outs[0].astype(cl) - ref).astype(np.float64)
    worst = float((err / bound).max())
    print('imaging_c64 nsrc=%d: worst err / bound = %.3f' % (nsrc, worst))
    assert (err <= bound).all(), worst
    # the complex128 kernel on the unpacked field gives the same bits: the rescaling is exact and the loop is k_imaging's
    dF, dG = torch.from_numpy(np.ascontiguousarray(UFh.T)).to(dev), torch.from_numpy(G0).to(dev)
    torch.cuda.synchronize(dev)
    op.imagingAccumulateDevice(dF.data_ptr(), dB.data_ptr(), nsrc, dS.data_ptr(), dG.data_ptr())
    assert np.array_equal(dG.cpu().numpy().view(np.float64), outs[0].view(np.float64))
    # a missing array or no column is refused before anything is launched (the pair takes no leading dimension and checks no alignment)
    i128, i64 = helm_lib.helm_imaging_accumulate_device, helm_lib.helm_imaging_accumulate_c64_device
    f, x, b, s, g = P(dF.data_ptr()), P(dE.data_ptr()), P(dB.data_ptr()), P(dS.data_ptr()), P(dG.data_ptr())
    assert i128(op.handle, None, b, nsrc, s, g) == -1 and i128(op.handle, f, None, nsrc, s, g) == -1 and i128(op.handle, f, b, 0, s, g) == -1
    assert i128(op.handle, f, b, nsrc, None, g) == -1 and i128(op.handle, f, b, nsrc, s, None) == -1 and i128(None, f, b, nsrc, s, g) == -1
    p = P(dP.data_ptr())
    assert i64(op.handle, None, x, b, nsrc, s, g) == -1 and i64(op.handle, p, None, b, nsrc, s, g) == -1 and i64(op.handle, p, x, None, nsrc, s, g) == -1
    assert i64(op.handle, p, x, b, 0, s, g) == -1 and i64(op.handle, p, x, b, nsrc, None, g) == -1 and i64(op.handle, p, x, b, nsrc, s, None) == -1


@pytest.mark.parametrize('nsrc', [1, 5, 13])
def test_sample_rows_c64_kernel_within_the_format_bound(helm_lib, op, nsrc):
    """helm_sample_rows_c64_device against out = beta out + alpha R_s u^_s from the unpacked u^, per output within
    2 (L + 4) 3.3 u (|alpha| sum_k |val_k||u^_k| + |beta||out0|) (the bound of test_sample_rows_against_numpy_within_the_format_bound), row stride nrec
    and 0, and a row-pointer sub-range for the batch of the last nsrc sources."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    dev = torch.device('cuda', op.device)
    N = op.nrow

    def sample(dU, dE, k, csr, row0, nrec, stride, alpha, beta, dout):
        _lib.check(helm_lib.helm_sample_rows_c64_device(op.handle, P(dU), P(dE), k, N, P(csr[0].data_ptr() + 8 * row0), P(csr[1].data_ptr()), P(csr[2].data_ptr()),
                                                        nrec, stride, alpha.real, alpha.imag, beta.real, beta.imag, P(dout)), op.handle)
    for name, sv in tm.moving_surveys():
        M = sv.stackedReceivers(0)
        nrec = sv.nrec
        rng = np.random.default_rng(300 * nsrc + nrec)
        Pk, e = pack_reference(wide_fields(rng, 13, N))
        Uh = unpack_reference(Pk, e)                                   # (N, 13)
        out0 = randc(rng, (nrec, nsrc))
        csr = tm.upload_csr(M, dev)
        dP, dE = torch.from_numpy(np.ascontiguousarray(Pk.T)).to(dev), torch.from_numpy(e).to(dev)
        for stride in (nrec, 0):
            blocks = [M[s * stride:s * stride + nrec] for s in range(nsrc)]
            RU = np.stack([np.asarray(b @ Uh[:, s]) for s, b in enumerate(blocks)], axis=1)
            absdot = np.stack([np.asarray(abs(b) @ np.abs(Uh[:, s])) for s, b in enumerate(blocks)], axis=1)
            L = np.stack([np.diff(b.indptr) for b in blocks], axis=1)
            for alpha, beta in tm.COEFFS:
                dout = torch.full((nrec, nsrc), float('nan'), dtype=torch.complex128, device=dev) if beta == 0 else torch.from_numpy(out0).to(dev)
                torch.cuda.synchronize(dev)
                sample(dP.data_ptr(), dE.data_ptr(), nsrc, csr, 0, nrec, stride, alpha, beta, dout.data_ptr())
                out = dout.cpu().numpy()
                ref, mag = (alpha * RU, abs(alpha) * absdot) if beta == 0 else (beta * out0 + alpha * RU, abs(alpha) * absdot + abs(beta) * np.abs(out0))
                assert np.isfinite(out.view(np.float64)).all(), (name, stride, alpha, beta)
                bound = 2 * (L + 4) * 3.3 * U_RND * mag
                err = np.abs(out - ref)
                worst = float((err[bound > 0] / bound[bound > 0]).max())
                print('sample_rows_c64 %s nsrc=%d stride=%d alpha=%s beta=%s: worst err / bound = %.3f' % (name, nsrc, stride, alpha, beta, worst))
                assert (err <= bound).all(), (name, stride, alpha, beta, worst)
        # the batch of the last nsrc sources: row pointer, fields and exponents all start at theirs
        c0 = 13 - nsrc
        dfull = torch.empty((nrec, 13), dtype=torch.complex128, device=dev)
        dpart = torch.full((nrec, nsrc), float('nan'), dtype=torch.complex128, device=dev)
        torch.cuda.synchronize(dev)
        sample(dP.data_ptr(), dE.data_ptr(), 13, csr, 0, nrec, nrec, 1.0 + 0j, 0j, dfull.data_ptr())
        sample(dP.data_ptr() + 8 * c0 * N, dE.data_ptr() + 4 * c0, nsrc, csr, c0 * nrec, nrec, nrec, 1.0 + 0j, 0j, dpart.data_ptr())
        assert np.array_equal(dpart.cpu().numpy(), dfull.cpu().numpy()[:, c0:])


# ---- the g6 survey -------------------------------------------------------------------------------------------------------------------------
def g6_pair(mode, **kw):
    if mode == 'relative':
        return tm.g6_pair(**kw)
    g, _ = tm.g6_config()
    return tm.g6_pair(geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), **kw)


def g6_goldens(mode):
    g = np.load(os.path.join(GOLD, 'g6_survey.npz'))
    if mode == 'fixed':
        return g['dpred'], g['resid'], g['g_u'], g['uF_f1_src3']
    g12 = np.load(os.path.join(GOLD, 'g12_moving_survey.npz'))
    return g['dpred_relative'], g12['resid'], g12['g_u'], g['uF_f1_src3']


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_g6_complex128_store_against_goldens_the_mux_pipeline_and_the_host_path(helm_lib, mode):
    from zephyr_amd.fieldstore import DeviceFields
    dgold, resid, g_u, uF13 = g6_goldens(mode)
    _, prob, sv = g6_pair(mode)
    _, probh, svh = g6_pair(mode, hostGradient=True)
    assert prob._deviceGradientAvailable() and not probh._deviceGradientAvailable()
    F = prob.fieldsDevice()
    assert isinstance(F, DeviceFields) and len(F) == sv.nfreq == 3 and F.dtype == 'complex128' and F.stamp == prob._modelStamp
    assert F.scale == complex(prob.system.scaleTerm) and sum(F.nbytes.values()) == 3 * 13 * prob.nrow * 16
    d0 = sv.dpred()
    dF = sv.dpred(u=F)
    assert np.array_equal(dF, d0)                          # the same launches on the same inputs, and solves are reproducible
    assert rel(dF, dgold) <= 1e-7
    gF = prob.Jtvec(None, resid, u=F)
    assert gF.shape == (prob.nrow,) and gF.dtype == np.float64
    assert rel(gF, g_u) <= 1e-6
    gh = probh.Jtvec(None, resid, u=probh.fields())
    assert gh.dtype == np.float64 and rel(gF, gh) <= 1e-9
    assert np.array_equal(prob.Jtvec(None, resid, u=F), gF)
    u1 = F[1]
    assert u1.shape == (prob.nrow, 13) and u1.dtype == np.complex128
    assert rel(u1[:, 3], uF13) <= 1e-7
    # iteration downloads: the host branch of Jtvec on the device problem's own fields
    gl = prob.Jtvec(None, resid, u=list(F))
    assert rel(gl, gF) <= 1e-9
    F.release()
    assert F.nbytes == {}
    with pytest.raises(ValueError):
        sv.dpred(u=F)
    del prob.factors, probh.factors


def test_counts_fields_solved_once_nothing_but_panels_and_the_gradient_comes_down(helm_lib, monkeypatch):
    """Patched as test_transfers_counted_no_wavefield_leaves_the_device does, plus the columns of every device solve: fieldsDevice solves nsrc columns per
    frequency and brings nothing down, dpred(u=F) solves nothing and brings down the panels, Jtvec(u=F) solves nsrc columns per frequency and brings
    down 16 N bytes once; no host-array solve anywhere.  The mux sequence next to it: 3 nsrc columns per frequency."""
    from zephyr_amd import _lib
    from zephyr_amd.discretization import BaseDiscretization
    monkeypatch.setenv('HELM_DEVICES', '0')
    counts = dict(solve=0, cols=[], down=[])
    real_solve, real_sd, real_fd, real_fdp = BaseDiscretization._solve, BaseDiscretization.solveDevice, _lib.from_device, _lib.from_device_pinned

    def solve(self, rhs, rows):
        counts['solve'] += 1
        return real_solve(self, rhs, rows)

    def solve_device(self, d_rhs, d_u, nrhs, *a, **k):
        counts['cols'].append(int(nrhs))
        return real_sd(self, d_rhs, d_u, nrhs, *a, **k)

    def counting(fn):
        def wrapped(t):
            counts['down'].append(t.numel() * t.element_size())
            return fn(t)
        return wrapped
    monkeypatch.setattr(BaseDiscretization, '_solve', solve)
    monkeypatch.setattr(BaseDiscretization, 'solveDevice', solve_device)
    monkeypatch.setattr(_lib, 'from_device', counting(real_fd))
    monkeypatch.setattr(_lib, 'from_device_pinned', counting(real_fdp))
    for mode in ('fixed', 'relative'):
        _, resid, _, _ = g6_goldens(mode)
        _, prob, sv = g6_pair(mode)
        N, nfreq, nsrc, nrec = prob.nrow, sv.nfreq, sv.nsrc, sv.nrec
        counts.update(solve=0, cols=[], down=[])
        F = prob.fieldsDevice()
        assert (counts['solve'], counts['cols'], counts['down']) == (0, [nsrc] * nfreq, [])
        counts.update(cols=[], down=[])
        sv.dpred(u=F)
        assert (counts['solve'], counts['cols'], sorted(counts['down'])) == (0, [], [nrec * nsrc * 16] * nfreq)
        counts.update(cols=[], down=[])
        prob.Jtvec(None, resid, u=F)
        assert (counts['solve'], counts['cols'], counts['down']) == (0, [nsrc] * nfreq, [N * 16])
        counts.update(cols=[], down=[])
        sv.dpred()
        prob.Jtvec(None, resid)
        assert counts['solve'] == 0 and sum(counts['cols']) == 3 * nsrc * nfreq
        F.release()
        del prob.factors


def test_two_workers_split_the_sources_and_agree_with_one(helm_lib, monkeypatch):
    'one frequency, two workers on GPU 0: the store is dealt 0:6 / 6:13, one slice per worker, and dpred(u=F) / Jtvec(u=F) run over those items'
    g, _ = tm.g6_config()
    one = dict(freqs=[float(g['freqs'][1])], sterms=g['sterms'][1:2])
    for mode in ('fixed', 'relative'):
        monkeypatch.setenv('HELM_DEVICES', '0')
        _, prob1, sv1 = g6_pair(mode, **one)
        F1 = prob1.fieldsDevice()
        assert [(c0, c1) for _, _, _, c0, c1 in F1.items] == [(0, 13)]
        d1 = sv1.dpred(u=F1)
        resid = randc(np.random.default_rng(8), d1.shape) * np.abs(d1).mean()
        g1 = prob1.Jtvec(None, resid, u=F1)
        u1 = F1[0]
        F1.release()
        del prob1.factors
        monkeypatch.setenv('HELM_DEVICES', '0,0')
        _, prob2, sv2 = g6_pair(mode, **one)
        assert len(prob2.system.devices) == 2
        F2 = prob2.fieldsDevice()
        assert [(w, dev, f, c0, c1) for w, dev, f, c0, c1 in F2.items] == [(0, 0, 0, 0, 6), (1, 0, 0, 6, 13)]
        assert F2.nbytes == {0: 13 * prob2.nrow * 16}
        assert rel(sv2.dpred(u=F2), d1) <= 1e-9
        assert rel(prob2.Jtvec(None, resid, u=F2), g1) <= 1e-9
        assert rel(F2[0], u1) <= 1e-9
        F2.release()
        del prob2.factors


def test_25d_store_holds_the_ky_sum(helm_lib):
    'g11, the ky sum formed in HBM by the composite: dpred(u=F) samples the sum where dpred() sums the samples (1e-9), Jtvec(u=F) against the host reduction'
    import zephyr_amd as za
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    g = np.load(os.path.join(GOLD, 'g11_25d_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=za.MiniZephyr25D, nky=int(g['nky']), parallel=False,
              sterms=g['sterms'], geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), rtol=1e-11)
    pairs = []
    for on in (True, False):
        cfg = dict(sc, kyOnDevice=on)
        prob, sv = Helm25DProblem(cfg), Helm25DSurvey(cfg)
        prob.pair(sv)
        assert prob._deviceGradientAvailable() is on
        pairs.append((prob, sv))
    (prob, sv), (probh, svh) = pairs
    with pytest.raises(RuntimeError):
        probh.fieldsDevice()                               # the host reduction: fields() stays the route
    F = prob.fieldsDevice()
    assert sum(F.nbytes.values()) == 2 * 5 * prob.nrow * 16
    d0 = sv.dpred()
    dF = sv.dpred(u=F)
    assert np.abs(d0).max() > 0 and rel(dF, d0) <= 1e-9
    assert rel(dF, g['dpred']) <= 1e-7
    resid = randc(np.random.default_rng(5), d0.shape) * np.abs(d0).mean()
    uh = probh.fields()
    gF, gh = prob.Jtvec(None, resid, u=F), probh.Jtvec(None, resid, u=uh)
    assert gF.dtype == np.float64 and rel(gF, gh) <= 1e-9
    assert rel(F[0], uh[0]) <= 1e-9
    F.release()
    del prob.factors, probh.factors


def test_complex64_store_against_the_complex128_store_within_the_format_bound(helm_lib):
    """g6 fixed.  Every stored component is within 2^-24 relative of the solved one, so |g64 - g128| <= 2 * 2^-24 * M per point with
    M = sum_f |scaler_f| sum_s |uF_s||uB_s| (host solves of qf and qb; the factor 2 covers the roundings of the sums themselves), and
    |d64 - d128| <= 2 * 2^-24 * (|R| |uF|) per datum."""
    _, resid, _, _ = g6_goldens('fixed')
    _, prob, sv = g6_pair('fixed')
    _, prob64, sv64 = g6_pair('fixed', fieldsDtype='complex64')
    _, probh, svh = g6_pair('fixed', hostGradient=True)
    F, F64 = prob.fieldsDevice(), prob64.fieldsDevice()
    assert F64.dtype == 'complex64' and sum(F64.nbytes.values()) == 3 * 13 * (prob.nrow * 8 + 4) and 2 * sum(F64.nbytes.values()) < 1.01 * sum(F.nbytes.values())
    g128, g64 = prob.Jtvec(None, resid, u=F), prob64.Jtvec(None, resid, u=F64)
    d128, d64 = sv.dpred(u=F), sv64.dpred(u=F64)
    assert g64.dtype == np.float64 and np.array_equal(prob64.Jtvec(None, resid, u=F64), g64)
    uF = probh.fields()
    qb = svh.getResidualSources(np.asarray(resid).reshape((sv.nrec, sv.nsrc, sv.nfreq)))
    M = np.zeros(prob.nrow)
    for ifreq, uB in probh._solveOwned(qb):
        M += np.abs(probh.gradientScaler(ifreq)) * (np.abs(uF[ifreq]) * np.abs(uB)).sum(axis=1)
    err = np.abs(g64 - g128)
    print('complex64 store: worst |g64 - g128| / (2 * 2^-24 M) = %.3f; rel = %.2e' % (float((err[M > 0] / (2 * 2.0 ** -24 * M[M > 0])).max()), rel(g64, g128)))
    assert (err <= 2 * 2.0 ** -24 * M).all()
    assert rel(g64, g128) > 0                              # (the packed store was read, not a complex128 copy)
    bound = np.stack([2 * 2.0 ** -24 * np.asarray(abs(svh.rVec(0, f)) @ np.abs(uF[f])) for f in range(sv.nfreq)], axis=2)
    derr = np.abs(d64 - d128).reshape(bound.shape)
    print('complex64 store: worst |d64 - d128| / bound = %.3f' % float((derr / bound).max()))
    assert (derr <= bound).all()
    # what comes down from the packed store is the unpacked field
    assert rel(F64[1], F[1]) <= 2.0 ** -23 and np.abs(F64[1] - F[1]).max() > 0
    F.release(), F64.release()
    del prob.factors, prob64.factors, probh.factors


def test_stale_fields_and_the_multiscale_pairing_are_refused(helm_lib):
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    g, prob, sv = g6_pair('fixed')
    F = prob.fieldsDevice()
    resid = g['resid']
    d = sv.dpred(u=F)
    prob.updateModel(g['c'])                               # the same model: the fields stay good
    assert np.array_equal(sv.dpred(u=F), d)
    prob.updateModel(g['c'] * 1.01)
    with pytest.raises(ValueError):
        sv.dpred(u=F)
    with pytest.raises(ValueError):
        prob.Jtvec(None, resid, u=F)
    F2 = prob.fieldsDevice(g['c'])                         # back to the first model: new fields, the old object stays refused
    assert np.array_equal(sv.dpred(u=F2), d)
    with pytest.raises(ValueError):
        sv.dpred(g['c'] * 1.01, u=F2)                      # a model handed to dpred itself counts too
    F.release(), F2.release()
    del prob.factors
    sc = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq)
    probm, svm = Helm2DProblem(sc), Helm2DMultiGridSurvey(sc)
    probm.pair(svm)
    with pytest.raises(NotImplementedError):
        probm.fieldsDevice()
