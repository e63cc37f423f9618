"""GPU: k_pseudo_hessian through its C entry points against the 80-bit evaluation of tests/pseudohessian_cases.py under its bound (all three modes, both store
formats, coefficients built in the kernel and read from the packed array, nsrc 1 / 4 / 5 / 33, padded columns, a non-zero H, with and without W, two runs the
same bits), what the entry points refuse, and the device routes of illumination(linearisation=, parameter=) on the 37 x 53 pair of full_cases against the
host route fed the same downloaded fields."""
import ctypes
import math

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import full_cases as xc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
LD, U64 = pc.LD, pc.U64
NSRCS = (1, 4, 5, 33)          # one column; a full group of PH_UNROLL; a partial second group; more groups than waves, the last one partial
GUARD, FILL, PAD = 131, 7.25, 37


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', sorted(pc.MODES))
@pytest.mark.parametrize('name', pc.HANDLES)
def test_kernel_against_the_80_bit_evaluation(helm_lib, name, mode):
    """H += alpha W (.) sum_s sum_j |E_i u_s|^2 on assembled handles (3 x 3, 4 x 4, 5 x 63, 33 x 125: nx either side of the 62-cell tile and into a third one,
    free-surface flags, ky, a damped frequency) per cell within c_ph(nsrc) 2^-53 (|H0| + alpha W M), plus (2 + 2^-24) 2^-24 alpha W M for the complex64 store.
    The columns are padded to ld = N + 37 with NaN, H starts non-zero between guard cells, W is given and NULL."""
    import torch
    from zephyr_amd import _lib
    sc, op, chain = pc.operator(name, mode, device=0)
    par, kmode = pc.MODES[mode][1], pc.MODES[mode][2]
    imode = op.PSEUDO_HESSIAN_MODES[kmode]
    N = sc['nz'] * sc['nx']
    ld = N + PAD
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(9)
    Wh = rng.uniform(0.5, 2.0, N)
    dW = torch.from_numpy(Wh).to(dev)
    dChain = None if chain is None else torch.from_numpy(np.ascontiguousarray(chain)).to(dev)
    d_chain = None if dChain is None else dChain.data_ptr()
    dE = torch.zeros(33 * N, dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(helm_lib.helm_pseudo_hessian_coefficients_device(op.handle, imode, None if d_chain is None else P(d_chain), P(dE.data_ptr())), op.handle)
    alpha = 0.37
    worst = {}
    for nsrc in NSRCS:
        u = pc.columns(N, nsrc, seed=nsrc)
        stored = np.full((nsrc, ld), complex(np.nan, np.nan))
        stored[:, :N] = np.conj(u).T                                             # (the store holds the conjugates of u^)
        dU = torch.from_numpy(stored).to(dev)
        dU32 = torch.zeros((nsrc, ld), dtype=torch.complex64, device=dev)
        dX = torch.zeros(nsrc, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        op.packDevice(dU.data_ptr(), nsrc, dU32.data_ptr(), dX.data_ptr(), rows=ld)
        HM = pc.exact(op, u, par, chain)                                         # (the 80-bit sums once per set of columns)
        for label, Wd, Wv in (('W', dW, Wh), ('noW', None, None)):
            H0 = rng.uniform(0.0, 1.0, N) * np.asarray(pc.combine(HM, alpha, Wv)[2], dtype=np.float64)
            H0[::3] = 0.0
            ref, mag, added = pc.combine(HM, alpha, Wv, H0)
            for fmt in ('c128', 'c64'):
                bound = pc.c_ph(nsrc) * U64 * mag + (pc.C64 * 2.0 ** -24 * added if fmt == 'c64' else 0)
                runs = {}
                for packed in (False, True):
                    for rep in range(2):
                        buf = torch.full((2 * GUARD + N,), FILL, dtype=torch.float64, device=dev)
                        buf[GUARD:GUARD + N] = torch.from_numpy(H0).to(dev)
                        torch.cuda.synchronize(dev)
                        d_h, d_w = buf.data_ptr() + 8 * GUARD, (None if Wd is None else Wd.data_ptr())
                        if not packed:
                            op.pseudoHessianAccumulateDevice(dU.data_ptr() if fmt == 'c128' else dU32.data_ptr(), nsrc, kmode, d_chain, alpha, d_w, d_h,
                                                             d_exp=None if fmt == 'c128' else dX.data_ptr(), rows=ld)
                        elif fmt == 'c128':
                            _lib.check(helm_lib.helm_pseudo_hessian_accumulate_packed_device(op.handle, P(dU.data_ptr()), nsrc, ld, imode, None, P(dE.data_ptr()), alpha,
                                                                                             None if d_w is None else P(d_w), P(d_h)), op.handle)
                        else:
                            _lib.check(helm_lib.helm_pseudo_hessian_accumulate_packed_c64_device(op.handle, P(dU32.data_ptr()), P(dX.data_ptr()), nsrc, ld, imode, None,
                                                                                                 P(dE.data_ptr()), alpha, None if d_w is None else P(d_w), P(d_h)), op.handle)
                        h = buf.cpu().numpy()
                        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + N:] == FILL)
                        runs[(packed, rep)] = h[GUARD:GUARD + N].copy()
                    assert np.array_equal(bits(runs[(packed, 0)]), bits(runs[(packed, 1)]))          # the same bits on every run
                    got = runs[(packed, 0)]
                    assert np.all(got >= H0) and np.any(got > H0)
                    key = '%s %s %s' % (fmt, 'packed' if packed else 'registers', label)
                    worst[key] = max(worst.get(key, 0.0), pc.worst_ratio(got, ref, bound))
    print('%s %s: worst err / bound %s' % (name, mode, ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    del op.factors


def test_entry_points_refuse_bad_arguments(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc, op, _ = pc.operator('even', 'explicit', device=0)
    N, nsrc = 16, 3
    dev = torch.device('cuda', 0)
    dU = torch.zeros((nsrc, N), dtype=torch.complex128, device=dev)
    dU32 = torch.zeros((nsrc, N), dtype=torch.complex64, device=dev)
    dX = torch.zeros(nsrc, dtype=torch.int32, device=dev)
    dW, dH, dC = (torch.zeros(N + 2, dtype=torch.float64, device=dev) for _ in range(3))
    torch.cuda.synchronize(dev)
    h, u, u32, x, w, e, c = op.handle, dU.data_ptr(), dU32.data_ptr(), dX.data_ptr(), dW.data_ptr(), dH.data_ptr(), dC.data_ptr()
    f128, f64 = helm_lib.helm_pseudo_hessian_accumulate_device, helm_lib.helm_pseudo_hessian_accumulate_c64_device
    assert f128(h, P(u), nsrc, N, 0, None, 1.0, P(w), P(e)) == 0 and f64(h, P(u32), P(x), nsrc, N, 2, P(c), 0.0, None, P(e)) == 0
    for bad in ((None, P(u), nsrc, N, 0, None, 1.0, P(w), P(e)), (h, None, nsrc, N, 0, None, 1.0, P(w), P(e)), (h, P(u), nsrc, N, 0, None, 1.0, P(w), None),
                (h, P(u), 0, N, 0, None, 1.0, P(w), P(e)), (h, P(u), nsrc, N - 1, 0, None, 1.0, P(w), P(e)), (h, P(u + 8), nsrc, N, 0, None, 1.0, P(w), P(e)),
                (h, P(u), nsrc, N, 0, None, 1.0, P(w + 4), P(e)), (h, P(u), nsrc, N, 0, None, 1.0, P(w), P(e + 4)), (h, P(u), nsrc, N, 0, None, -1.0, P(w), P(e)),
                (h, P(u), nsrc, N, 0, None, math.nan, P(w), P(e)), (h, P(u), nsrc, N, 3, None, 1.0, P(w), P(e)), (h, P(u), nsrc, N, -1, None, 1.0, P(w), P(e)),
                (h, P(u), nsrc, N, 2, None, 1.0, P(w), P(e)), (h, P(u), nsrc, N, 0, P(c), 1.0, P(w), P(e)), (h, P(u), nsrc, N, 1, P(c), 1.0, P(w), P(e)),
                (h, P(u), nsrc, N, 2, P(c + 4), 1.0, P(w), P(e)), (h, P(u), nsrc, N, 0, None, 1.0, P(e), P(e)), (h, P(u), nsrc, N, 2, P(e + 8), 1.0, P(w), P(e))):
        assert f128(*bad) == -1, bad
    for bad in ((h, P(u32), None, nsrc, N, 0, None, 1.0, P(w), P(e)), (h, P(u32 + 4), P(x), nsrc, N, 0, None, 1.0, P(w), P(e)),
                (h, P(u32), P(x + 2), nsrc, N, 0, None, 1.0, P(w), P(e)), (h, None, P(x), nsrc, N, 0, None, 1.0, P(w), P(e)),
                (h, P(u32), P(x), nsrc, N - 1, 0, None, 1.0, P(w), P(e))):
        assert f64(*bad) == -1, bad
    assert np.all(dH.cpu().numpy() == 0.0)                                      # (the fields were zero, and a refused call launches nothing)
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert raw, _lib.last_error(None)
    big = torch.zeros(4 * 108, dtype=torch.complex128, device=dev)
    hh = torch.zeros(108, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert f128(raw, P(big.data_ptr()), 2, 108, 0, None, 1.0, None, P(hh.data_ptr())) == -3          # (no assembled operator: HELM_ERR_STATE)
    helm_lib.helm_destroy(raw)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    Ne = int(helm_lib.helm_num_points(eu))
    ue, he = torch.zeros(Ne, dtype=torch.complex128, device=dev), torch.zeros(Ne, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert f128(eu, P(ue.data_ptr()), 1, Ne, 0, None, 1.0, None, P(he.data_ptr())) == -4             # (HELM_ERR_UNSUPPORTED)
    helm_lib.helm_destroy(eu)
    del op.factors


# ---- 2. the routes ------------------------------------------------------------------------------------------------------------------------------------------
ROUTES = [('explicit', dict(linearisation='full')), ('gardner', dict(linearisation='full')), ('rho', dict(linearisation='operator', parameter='rho'))]


def host_and_bound(prob, fields, kw, launches=1):
    """the host route fed the fields given, rows per frequency, and the bound on |device - host| per row: both are fp64 evaluations of the same sums, each
    within c_ph(nsrc) 2^-53 |scaleTerm|^2 M_f of the exact value (pseudohessian_cases); `launches` partials of a frequency add one rounding each, and 1 / rho^4
    and |scaleTerm|^2 are made twice (8)."""
    st = complex(prob.system.scaleTerm)
    par = kw.get('parameter', 'c')
    chain = prob._gardnerChain() if par == 'c' else None
    rows = prob.illumination(u=fields, perFreq=True, **kw)
    mag = np.stack([abs(st) ** 2 * fr.pseudoHessianDiagonal(sub, np.conj(np.asarray(uf) / st), par, chain, magnitude=True)
                    for sub, uf in zip(prob.system.subProblems, fields)])
    ns = np.asarray(fields[0]).shape[1]
    return rows, 2 * (pc.c_ph(ns) + launches + 8) * U64 * mag


@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('mode,kw', ROUTES, ids=[r[0] for r in ROUTES])
def test_routes_against_the_host_route_fed_the_downloaded_fields(helm_lib, monkeypatch, mode, kw, fmt):
    """u = F (either store), perFreq, u = None and repeated calls on the 37 x 53 pair (HD: a complex scaleTerm).  F[f] downloads what the kernel reads -- the
    complex64 store unpacked -- so only the arithmetic of the kernel differs from the host route on u = [F[f] ...] and the kernel's bound applies."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', True, density=pc.MODES[mode][0], device=True, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    fields = [F[f] for f in range(sv.nfreq)]
    rows, bound = host_and_bound(prob, fields, kw)
    RF = prob.illumination(u=F, perFreq=True, **kw)
    HF = prob.illumination(u=F, **kw)
    assert RF.shape == (sv.nfreq, prob.nrow) and HF.shape == (prob.nrow,) and HF.dtype == np.float64 and np.all(HF >= 0)
    ratio = pc.worst_ratio(RF, rows.astype(LD), bound.astype(LD))
    print('%s %s: illumination(u=F) rows, worst |device - host| / bound = %.4f' % (mode, fmt, ratio))
    assert ratio <= 1.0
    assert pc.worst_ratio(HF, rows.sum(axis=0).astype(LD), (bound.sum(axis=0) + 2 * sv.nfreq * U64 * rows.sum(axis=0)).astype(LD)) <= 1.0
    assert np.array_equal(bits(prob.illumination(u=F, **kw)), bits(HF))                                  # the same bits on every run
    if fmt == 'complex128':
        H0 = prob.illumination(**kw)                                                                     # solved into the workspace, accumulated, dropped
        print('%s: illumination() bit-identical to illumination(u=F): %s' % (mode, np.array_equal(H0, HF)))
        assert pc.worst_ratio(H0, rows.sum(axis=0).astype(LD), (bound.sum(axis=0) + 2 * sv.nfreq * U64 * rows.sum(axis=0)).astype(LD)) <= 1.0
        assert ac.rel(prob.illumination(u=F, kind='energy'), HF) > 1e-3                                  # (not the plain energy)
    F.release()
    del prob.factors


def test_receiver_side_and_two_workers(helm_lib, monkeypatch):
    """side='receiver' against the host route of the same problem (its own solves: the 1e-12 of tests/test_gpu_illumination.py, where no field comes down), and
    two workers on GPU 0 splitting the columns of one frequency against the host route fed the downloaded fields: two partials, one host addition more."""
    kw = dict(linearisation='full')
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', True, device=True)
    probh, _ = xc.pair('fixed', True, device=True, hostGradient=True)
    HR = prob.illumination(side='receiver', perFreq=True, **kw)
    assert HR.shape == (sv.nfreq, prob.nrow) and np.all(HR >= 0) and HR.max() > 0
    assert ac.rel(HR, probh.illumination(side='receiver', perFreq=True, **kw)) <= 1e-12
    assert ac.rel(HR.sum(axis=0), prob.illumination(**kw)) > 1e-3                                         # (not the source side)
    del prob.factors, probh.factors
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = xc.fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[xc.fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]))
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob2, sv2 = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob2.pair(sv2)
    assert len(prob2.system.devices) == 2
    F2 = prob2.fieldsDevice()
    assert len(F2.items) == 2
    rows, bound = host_and_bound(prob2, [F2[0]], kw, launches=2)
    for H in (prob2.illumination(u=F2, **kw), prob2.illumination(**kw)):
        assert pc.worst_ratio(H, rows[0].astype(LD), bound[0].astype(LD)) <= 1.0
    F2.release()
    del prob2.factors


def test_operator_route_is_the_energy_kernel_with_the_closed_form_weight(helm_lib, monkeypatch):
    """linearisation='operator', parameter='c' launches helm_energy_accumulate_device: the result is that kernel's on the same store with the weight
    |d K / d c|^2 S of frechet.operatorPseudoHessianWeight, up to the roundings of the weight (made on the device as 4 |omega_d^2|^2 |scaleTerm|^2 S / |c^3 rho|^2:
    the 32 of test_gpu_illumination's WEIGHT_SLACK) and of the sum ((nsrc + 7) per launch) -- every term is non-negative, so the bound is relative"""
    import torch
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', True, device=True)
    calls = []
    for sub in prob.system.subProblems:
        orig = sub.energyAccumulateDevice
        monkeypatch.setattr(sub, 'energyAccumulateDevice', lambda *a, _o=orig, **k: (calls.append(1), _o(*a, **k))[1])
        monkeypatch.setattr(sub, 'pseudoHessianAccumulateDevice', lambda *a, **k: pytest.fail('the closed form needs no new kernel'))
    F = prob.fieldsDevice()
    Ho = prob.illumination(u=F, linearisation='operator')
    assert len(calls) == len(F.items)
    st = complex(prob.system.scaleTerm)
    dev = torch.device('cuda', 0)
    E = torch.zeros(prob.nrow, dtype=torch.float64, device=dev)
    for _, _, ifreq, c0, c1 in F.items:
        op = prob.system.subProblems[ifreq]
        W = torch.from_numpy(fr.operatorPseudoHessianWeight(op)).to(dev)
        torch.cuda.synchronize(dev)
        d_u, d_exp = F.pointers(ifreq, c0)
        op.energyAccumulateDevice(d_u, c1 - c0, abs(st) ** 2, W.data_ptr(), E.data_ptr(), d_exp=d_exp, rows=int(op.nrow))
    want = E.cpu().numpy()
    slack = 2 * (len(F.items) * (sv.nsrc + 7) + 32) * U64
    assert np.all(np.abs(Ho - want) <= slack * want) and want.max() > 0
    assert ac.rel(Ho, prob.illumination(u=[F[f] for f in range(sv.nfreq)], linearisation='operator')) <= 1e-14
    F.release()
    del prob.factors
