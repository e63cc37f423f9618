"""GPU: the per-cell 2 x 2 blocks of the joint (c, rho) Hessian -- k_gauss_newton_blocks and k_pseudo_hessian_blocks against the 80-bit evaluations of
tests/blocks_cases.py under its bounds (tile edges, both store formats, padded columns, ldH > N, non-zero outputs between guard words, two runs the same bits),
what the entry points refuse, the device routes of hessianBlocks on the 37 x 53 pair against the host route fed the downloaded fields and against the cross
entries of the device Hvec(parameter='joint'), and the existing routes before and after a blocks call."""
import ctypes
import math

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import blocks_cases as bc
from tests import full_cases as xc
from tests import gaussnewton_cases as gc
from tests import pseudohessian_cases as pc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
LD, U64 = bc.LD, bc.U64
GUARD, PAD, HPAD = 131, 37, 5
FILL = 7.25
NSRCS = (1, 4, 5, 33)          # one column, a full group, a partial second group, more groups than waves with the last one partial
ROUTE_TOL = 1e-6               # the route tolerance of tests/test_gpu_gaussnewton.py
EIGHT = [0, 3, 10, 12, 17, 21, 27, 33]          # of gaussnewton_cases.cells_37x53, as tests/test_gpu_gaussnewton.py


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def start_rows(rng, mag0, N):
    "H0 (3, N) of the size of what is added, any sign in the middle row, a third of it exactly zero"
    H0 = rng.uniform(0.0, 1.0, (3, N)) * np.asarray(mag0, dtype=np.float64)
    H0[1] *= rng.choice([-1.0, 1.0], N)
    H0[:, ::3] = 0.0
    return H0


def run_rows(torch, dev, H0, N, call):
    "the three rows after call(d_h, ldh) on a buffer [guard | row 0 | pad | row 1 | pad | row 2 | guard]: guards and pads must keep their fill"
    ldh = N + HPAD
    buf = torch.full((2 * GUARD + 2 * ldh + N,), FILL, dtype=torch.float64, device=dev)
    for a in range(3):
        buf[GUARD + a * ldh:GUARD + a * ldh + N] = torch.from_numpy(np.ascontiguousarray(H0[a])).to(dev)
    torch.cuda.synchronize(dev)
    call(buf.data_ptr() + 8 * GUARD, ldh)
    h = buf.cpu().numpy()
    body = h[GUARD:GUARD + 2 * ldh + N]
    assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + 2 * ldh + N:] == FILL)
    assert np.all(body[N:ldh] == FILL) and np.all(body[ldh + N:2 * ldh] == FILL)
    return np.stack([body[a * ldh:a * ldh + N] for a in range(3)])


# ---- 1. k_gauss_newton_blocks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin', sorted(bc.LINS))
@pytest.mark.parametrize('name', pc.HANDLES)
def test_gauss_newton_blocks_kernel_against_the_80_bit_evaluation(helm_lib, name, lin):
    """The three rows on the four assembled handles of density_cases.OPERATOR_CASES (3 x 3, 4 x 4, 5 x 63, 33 x 125: free-surface flags, dx != dz, ky, a damped
    frequency, cell counts that are no multiple of 64), both values of `stretch`, per cell and row within C_GNB 2^-53 (|H0| + alpha M).  The planes are lag
    products of random columns, conjugated as the stored fields are, NaN where k_lag_gram never writes; H starts non-zero, alpha != 1, ldH = N + 5."""
    import torch
    sc, op, _ = pc.operator(name, 'explicit', device=0)
    nz, nx = sc['nz'], sc['nx']
    N = nz * nx
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(11)
    Cu, Cg, touched = gc.combine_inputs(nz, nx, seed=N)
    stored = []
    for C in (Cu, Cg):
        d = np.conj(C)
        d[~touched] = complex(np.nan, np.nan)
        stored.append(torch.from_numpy(d.ravel()).to(dev))
    alpha = 0.37
    ref0, mag0 = bc.gn_reference(op, Cu, Cg, lin, alpha, np.zeros((3, N)))
    H0 = start_rows(rng, mag0, N)
    ref, mag = ref0 + H0.astype(LD), mag0 + np.abs(H0).astype(LD)
    runs = [run_rows(torch, dev, H0, N, lambda d_h, ldh: op.gaussNewtonBlocksDevice(bc.LINS[lin], stored[0].data_ptr(), stored[1].data_ptr(), alpha, d_h, ldh=ldh))
            for _ in range(2)]
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    assert np.all(np.isfinite(runs[0])) and np.any(runs[0][0] > H0[0]) and np.any(runs[0][1] != H0[1])
    worst = bc.worst_rows(runs[0], ref, bc.C_GNB * U64 * mag)
    print('%s %s: k_gauss_newton_blocks worst err / bound per row %s' % (name, lin, ' '.join('%.4f' % w for w in worst)))
    assert max(worst) <= 1.0, worst
    del op.factors


# ---- 2. k_pseudo_hessian_blocks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin', sorted(bc.LINS))
@pytest.mark.parametrize('name', pc.HANDLES)
def test_pseudo_hessian_blocks_kernel_against_the_80_bit_evaluation(helm_lib, name, lin):
    """The same handles (widths either side of the 62-cell tile and into a third one), nsrc in (1, 4, 5, 33), both store formats, columns of magnitudes 1e-3 .. 1e3
    padded to ld = N + 37 with NaN: per cell and row within c_phb(nsrc) 2^-53 (|H0| + alpha M), plus (2 + 2^-24) 2^-24 alpha M for the complex64 store"""
    import torch
    sc, op, _ = pc.operator(name, 'explicit', device=0)
    N = sc['nz'] * sc['nx']
    ld = N + PAD
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(9)
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
        ref0, mag0, added = bc.ph_reference(op, u, lin, alpha, np.zeros((3, N)))
        H0 = start_rows(rng, mag0, N)
        ref, mag = ref0 + H0.astype(LD), mag0 + np.abs(H0).astype(LD)
        for fmt in ('c128', 'c64'):
            bound = bc.c_phb(nsrc) * U64 * mag + (bc.C64 * 2.0 ** -24 * added if fmt == 'c64' else 0)
            call = lambda d_h, ldh: op.pseudoHessianBlocksDevice(dU.data_ptr() if fmt == 'c128' else dU32.data_ptr(), nsrc, bc.LINS[lin], alpha, d_h, ldh=ldh,
                                                                 d_exp=None if fmt == 'c128' else dX.data_ptr(), rows=ld)
            runs = [run_rows(torch, dev, H0, N, call) for _ in range(2)]
            assert np.array_equal(bits(runs[0]), bits(runs[1]))                  # the same bits on every run
            assert np.all(np.isfinite(runs[0])) and np.all(runs[0][2] >= H0[2]) and np.any(runs[0][1] != H0[1])
            for a, w in enumerate(bc.worst_rows(runs[0], ref, bound)):
                key = '%s row %d' % (fmt, a)
                worst[key] = max(worst.get(key, 0.0), w)
    print('%s %s: k_pseudo_hessian_blocks worst err / bound %s' % (name, lin, ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    del op.factors


# ---- 3. what the entry points refuse ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(helm_lib):
    import torch
    from zephyr_amd import _lib
    sc, op, _ = pc.operator('even', 'explicit', device=0)
    N, nsrc = 16, 3
    dev = torch.device('cuda', 0)
    dCu, dCg = (torch.zeros(13 * N + 2, dtype=torch.complex128, device=dev) for _ in range(2))
    dU = torch.zeros((nsrc, N), dtype=torch.complex128, device=dev)
    dU32 = torch.zeros((nsrc, N), dtype=torch.complex64, device=dev)
    dX = torch.zeros(nsrc, dtype=torch.int32, device=dev)
    dH = torch.zeros(3 * N + 2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    h, cu, cg, u, u32, x, e = op.handle, dCu.data_ptr(), dCg.data_ptr(), dU.data_ptr(), dU32.data_ptr(), dX.data_ptr(), dH.data_ptr()
    g, f128, f64 = helm_lib.helm_gauss_newton_blocks_device, helm_lib.helm_pseudo_hessian_blocks_device, helm_lib.helm_pseudo_hessian_blocks_c64_device
    for stretch in (0, 1):
        assert g(h, stretch, P(cu), P(cg), 1.0, P(e), N) == 0 and f128(h, P(u), nsrc, N, stretch, 1.0, P(e), N) == 0
        assert f64(h, P(u32), P(x), nsrc, N, stretch, 0.0, P(e), N) == 0
    for bad in ((None, 1, P(cu), P(cg), 1.0, P(e), N), (h, 1, None, P(cg), 1.0, P(e), N), (h, 1, P(cu), None, 1.0, P(e), N), (h, 1, P(cu), P(cg), 1.0, None, N),
                (h, 2, P(cu), P(cg), 1.0, P(e), N), (h, -1, P(cu), P(cg), 1.0, P(e), N), (h, 1, P(cu), P(cg), -1.0, P(e), N), (h, 1, P(cu), P(cg), math.nan, P(e), N),
                (h, 1, P(cu + 8), P(cg), 1.0, P(e), N), (h, 1, P(cu), P(cg + 8), 1.0, P(e), N), (h, 1, P(cu), P(cg), 1.0, P(e + 4), N),
                (h, 1, P(cu), P(cg), 1.0, P(e), N - 1), (h, 1, P(cu), P(cg), 1.0, P(cu), N), (h, 1, P(cu), P(cg), 1.0, P(cg + 16), N),
                (h, 1, P(cu), P(cg), 1.0, P(cu - 8 * 2 * N - 8), N)):          # (the third row reaches into the planes)
        assert g(*bad) == -1, bad
    for bad in ((None, P(u), nsrc, N, 1, 1.0, P(e), N), (h, None, nsrc, N, 1, 1.0, P(e), N), (h, P(u), nsrc, N, 1, 1.0, None, N), (h, P(u), 0, N, 1, 1.0, P(e), N),
                (h, P(u), nsrc, N - 1, 1, 1.0, P(e), N), (h, P(u + 8), nsrc, N, 1, 1.0, P(e), N), (h, P(u), nsrc, N, 1, 1.0, P(e + 4), N),
                (h, P(u), nsrc, N, 1, -1.0, P(e), N), (h, P(u), nsrc, N, 1, math.nan, P(e), N), (h, P(u), nsrc, N, 2, 1.0, P(e), N), (h, P(u), nsrc, N, -1, 1.0, P(e), N),
                (h, P(u), nsrc, N, 1, 1.0, P(e), N - 1), (h, P(u), nsrc, N, 1, 1.0, P(u), N), (h, P(u), nsrc, N, 1, 1.0, P(u - 8 * 2 * N - 8), N)):
        assert f128(*bad) == -1, bad
    for bad in ((h, P(u32), None, nsrc, N, 1, 1.0, P(e), N), (h, P(u32 + 4), P(x), nsrc, N, 1, 1.0, P(e), N), (h, P(u32), P(x + 2), nsrc, N, 1, 1.0, P(e), N),
                (h, None, P(x), nsrc, N, 1, 1.0, P(e), N), (h, P(u32), P(x), nsrc, N - 1, 1, 1.0, P(e), N), (h, P(u32), P(x), nsrc, N, 1, 1.0, P(e), N - 1)):
        assert f64(*bad) == -1, bad
    assert np.all(dH.cpu().numpy() == 0.0)                                      # (the inputs were zero, and a refused call launches nothing)
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert raw, _lib.last_error(None)
    big = torch.zeros(13 * 108, dtype=torch.complex128, device=dev)
    hh = torch.zeros(3 * 108, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert g(raw, 1, P(big.data_ptr()), P(big.data_ptr()), 1.0, P(hh.data_ptr()), 108) == -3          # (no assembled operator: HELM_ERR_STATE)
    assert f128(raw, P(big.data_ptr()), 2, 108, 1, 1.0, P(hh.data_ptr()), 108) == -3
    helm_lib.helm_destroy(raw)
    for nz, nx in ((2, 40), (40, 2)):          # nz or nx below 3: the library makes no such handle, so the entry points' own check stands behind this one
        assert not helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, nz, nx, 10., 10., 0, (ctypes.c_int * 4)(0, 0, 0, 0))
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    Ne = int(helm_lib.helm_num_points(eu))
    ce, he = torch.zeros(13 * Ne, dtype=torch.complex128, device=dev), torch.zeros(3 * Ne, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert g(eu, 1, P(ce.data_ptr()), P(ce.data_ptr()), 1.0, P(he.data_ptr()), Ne) == -4             # (HELM_ERR_UNSUPPORTED)
    assert f128(eu, P(ce.data_ptr()), 1, Ne, 1, 1.0, P(he.data_ptr()), Ne) == -4
    helm_lib.helm_destroy(eu)
    del op.factors


# ---- 4. the routes --------------------------------------------------------------------------------------------------------------------------------------------
ROUTES = [('full', False, 'complex128'), ('full', True, 'complex64'), ('operator', True, 'complex128'), ('operator', False, 'complex64')]


def route_errors(got, want):
    "rows 0 and 2 per cell and relative, row 1 per cell on sqrt(B0 B2) of the cell (of `want`)"
    return gc.rel(got[0], want[0]), bc.cross_error(got[1], want[1], np.sqrt(want[0] * want[2])), gc.rel(got[2], want[2])


@pytest.mark.parametrize('lin,hd,fmt', ROUTES, ids=['%s-%s-%s' % (l, 'hd' if h else 'mz', f) for l, h, f in ROUTES])
def test_routes_against_the_host_route_and_against_hvec(helm_lib, monkeypatch, lin, hd, fmt):
    """hessianBlocks(u=F) on the 37 x 53 pair with a fixed array, MiniZephyr and MiniZephyrHD (a complex scaleTerm), both stores: within 1e-6 (the route tolerance
    of tests/test_gpu_gaussnewton.py) of the host route fed the downloaded fields -- rows 0 and 2 per cell and relative, row 1 per cell on sqrt(B0 B2) --, perFreq
    rows that sum to the total, the same bits twice and (complex128 store) from u = None; B[1] at eight cells within the same 1e-6 of both cross entries of the
    device Hvec(parameter='joint'), in that test's norm (the largest difference over the cells on the largest sqrt(B0 B2)).  The pseudo-Hessian kind likewise."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', hd, device=True, rtol=1e-11, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    down = [F[f] for f in range(sv.nfreq)]
    for kind in ('gaussNewton', 'pseudoHessian'):
        kw = dict(kind=kind, linearisation=lin)
        B = prob.hessianBlocks(u=F, **kw)
        assert B.shape == (3, prob.nrow) and B.dtype == np.float64 and bc.gram_properties(B, slack=1e-9) and B[0].max() > 0 and B[1].min() < 0 < B[1].max()
        errs = route_errors(B, prob.hessianBlocks(u=down, **kw))
        rows = prob.hessianBlocks(u=F, perFreq=True, **kw)
        assert rows.shape == (sv.nfreq, 3, prob.nrow) and float(np.max(np.abs(rows.sum(axis=0) - B) / np.abs(rows).sum(axis=0).max(axis=1, keepdims=True))) <= 1e-14
        assert np.array_equal(bits(prob.hessianBlocks(u=F, **kw)), bits(B))                                # the same bits on every run
        if fmt == 'complex128':
            assert np.array_equal(bits(prob.hessianBlocks(**kw)), bits(B))                                 # solved into HBM, read and dropped
        print('%s %s hd=%s %s: |device - host| rows 0 / 1 / 2 %.2e / %.2e / %.2e' % ((kind, lin, hd, fmt) + errs))
        assert max(errs) <= ROUTE_TOL
        if kind == 'gaussNewton':
            cells = [gc.cells_37x53()[k] for k in EIGHT]
            a, b = bc.hvec_cross(prob, F, cells, lin)
            scale = float(np.sqrt(B[0][cells] * B[2][cells]).max())
            e_hvec = max(float(np.max(np.abs(B[1][cells] - a))), float(np.max(np.abs(B[1][cells] - b)))) / scale
            print('    B[1] against the device Hvec at eight cells: %.2e of the largest sqrt(B0 B2)' % e_hvec)
            assert e_hvec <= ROUTE_TOL
            assert ac.rel(prob.hessianBlocks(u=F, kind='pseudoHessian', linearisation=lin), B) > 1e-3    # (not the pseudo-Hessian)
    F.release()
    del prob.factors


def test_two_workers_moving_array_receiver_side_and_refusals(helm_lib, monkeypatch):
    """two workers on GPU 0 with half the sources of one frequency each (every worker makes its own Gamma_f, the partials are added on the host); the
    pseudo-Hessian kind on an array that moves with the source and with side='receiver' against the host route of the same problem; the device-path refusals"""
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = xc.fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[xc.fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    for kind in ('gaussNewton', 'pseudoHessian'):
        host = prob.hessianBlocks(u=[F[0]], kind=kind)
        for B in (prob.hessianBlocks(u=F, kind=kind), prob.hessianBlocks(kind=kind)):
            assert max(route_errors(B, host)) <= ROUTE_TOL
    F.release()
    del prob.factors
    monkeypatch.setenv('HELM_DEVICES', '0')
    moving, _ = xc.pair('relative', False, device=True)
    movingh, _ = xc.pair('relative', False, device=True, hostGradient=True)
    assert max(route_errors(moving.hessianBlocks(kind='pseudoHessian'), movingh.hessianBlocks(kind='pseudoHessian'))) <= ROUTE_TOL
    with pytest.raises(ValueError, match='fixed receiver arrays'):
        moving.hessianBlocks()
    del moving.factors, movingh.factors
    fixed, _ = xc.pair('fixed', False, device=True)
    fixedh, _ = xc.pair('fixed', False, device=True, hostGradient=True)
    R = fixed.hessianBlocks(kind='pseudoHessian', side='receiver', linearisation='operator')
    assert max(route_errors(R, fixedh.hessianBlocks(kind='pseudoHessian', side='receiver', linearisation='operator'))) <= ROUTE_TOL
    with pytest.raises(ValueError, match='side'):
        fixed.hessianBlocks(side='receiver')
    with pytest.raises(ValueError, match='kind'):
        fixed.hessianBlocks(kind='energy')
    with pytest.raises(ValueError, match='joint'):
        fixed.hessianBlocks(linearisation='scaler')
    gardner, _ = xc.pair('fixed', False, density=False, device=True)
    with pytest.raises(NotImplementedError, match='rho'):
        gardner.hessianBlocks()
    del fixed.factors, fixedh.factors


# ---- 5. the existing routes stay as they are ------------------------------------------------------------------------------------------------------------------
def test_existing_routes_give_the_same_bits_before_and_after_a_blocks_call(helm_lib, monkeypatch):
    """illumination of every kind, the joint Jtvec and Hvec, then three blocks calls, then the first set again: the same bits.  (The 'scaler' pseudo-Hessian is
    left out: this case has a damped frequency, whose complex omega that route does not take.)"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', True, device=True, rtol=1e-11)
    F = prob.fieldsDevice()
    rng = np.random.default_rng(5)
    r = ac.randc(rng, sv.nD)
    v = rng.uniform(-1.0, 1.0, 2 * prob.nrow)

    def existing():
        out = [prob.illumination(u=F, kind='energy'), prob.illumination(u=F, linearisation='operator'), prob.illumination(u=F, linearisation='full'),
               prob.illumination(u=F, linearisation='operator', parameter='rho'), prob.illumination(u=F, kind='gaussNewton', linearisation='full'),
               prob.illumination(u=F, kind='gaussNewton', linearisation='operator', parameter='rho'),
               prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full', parameter='joint'),
               prob.Hvec(None, v, u=F, linearisation='full', parameter='joint'), prob.Hvec(None, v[:prob.nrow], u=F, linearisation='operator')]
        return [np.array(x) for x in out]
    before = existing()
    for kw in (dict(kind='gaussNewton'), dict(kind='pseudoHessian'), dict(kind='gaussNewton', linearisation='operator', perFreq=True)):
        assert np.all(np.isfinite(prob.hessianBlocks(u=F, **kw)))
    after = existing()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    F.release()
    del prob.factors
