"""GPU: the exact diagonal of the Gauss-Newton Hessian -- k_lag_gram through both entry points and k_gauss_newton_diagonal in every mode against the 80-bit
evaluations of tests/gaussnewton_cases.py under its bounds (tile edges, both store formats, padded columns, non-zero outputs between guard words, two runs the
same bits), what the entry points refuse, and the device routes of illumination(kind='gaussNewton') on the 37 x 53 pair against the host route fed the
downloaded fields and against e_i . Hvec(e_i) on the device."""
import ctypes
import math

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import full_cases as xc
from tests import gaussnewton_cases as gc
from tests import pseudohessian_cases as pc
from zephyr_amd import frechet as fr

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
LD, U64 = gc.LD, gc.U64
GUARD, PAD = 131, 37


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class RawHandle(object):
    'a library handle of a grid, created and never assembled: k_lag_gram reads the grid and the stream of a handle, not its operator'

    def __init__(self, lib, nz, nx):
        from zephyr_amd import _lib
        self.lib, self.device = lib, 0
        self.handle = lib.helm_create(0, _lib.HELM_MINIZEPHYR, nz, nx, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
        assert self.handle, _lib.last_error(None)

    def close(self):
        self.lib.helm_destroy(self.handle)


# ---- 1. k_lag_gram ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('case', gc.GRAM_CASES, ids=['%dx%dx%d' % c for c in gc.GRAM_CASES])
def test_lag_gram_against_the_80_bit_evaluation(helm_lib, case, fmt):
    """C_l += sum_s U_s conj(shift_l U_s) per component within c_gram(nsrc) 2^-53 (|C0| + sum |u||u'|), plus (2 + 2^-24) 2^-24 of the added magnitude for the
    complex64 store.  Widths 59 .. 64 lie either side of the 60-cell tile, 121 and 125 reach a third one; 3 x 3 and 33 x 3 have lags that leave the grid.  The
    columns have very different sizes and are padded to ld = N + 37; C starts non-zero between guard words; entries whose partner lies outside the grid keep
    their bits; two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference
    nz, nx, nsrc = case
    op = RawHandle(helm_lib, nz, nx)
    dev = torch.device('cuda', 0)
    N = nz * nx
    ld = N + PAD
    U, C0 = gc.gram_inputs(nz, nx, nsrc, seed=100 * nz + nx + nsrc)
    if fmt == 'complex64':
        Pk, e = pack_reference(np.ascontiguousarray(U.T))
        pad = np.zeros((nsrc, ld), dtype=np.complex64)
        pad[:, :N] = Pk.T
        dU, dE = torch.from_numpy(pad).to(dev), torch.from_numpy(e).to(dev)
    else:
        pad = np.zeros((nsrc, ld), dtype=np.complex128)
        pad[:, :N] = U
        dU, dE = torch.from_numpy(pad).to(dev), None
    fill = complex(7.0, -3.0)
    runs = []
    for _ in range(2):
        buf = torch.full((2 * GUARD + 13 * N,), fill, dtype=torch.complex128, device=dev)
        buf[GUARD:GUARD + 13 * N] = torch.from_numpy(C0.ravel()).to(dev)
        torch.cuda.synchronize(dev)
        d_c = P(buf.data_ptr() + 16 * GUARD)
        if fmt == 'complex64':
            _lib.check(helm_lib.helm_lag_gram_accumulate_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), nsrc, ld, d_c), op.handle)
        else:
            _lib.check(helm_lib.helm_lag_gram_accumulate_device(op.handle, P(dU.data_ptr()), nsrc, ld, d_c), op.handle)
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == fill) and np.all(h[GUARD + 13 * N:] == fill)
        runs.append(h[GUARD:GUARD + 13 * N].reshape((13, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    touched = gc.gram_touched(nz, nx)
    assert np.array_equal(bits(runs[0][~touched]), bits(C0[~touched]))                  # (entries whose partner is outside the grid are not written)
    assert touched[0].all() and np.all(runs[0][touched] != C0[touched])
    ref, mag, added = gc.gram_reference(C0, U, nz, nx)
    bound = gc.c_gram(nsrc) * U64 * mag + (gc.C64 * 2.0 ** -24 * added if fmt == 'complex64' else 0)
    worst = dc.worst_ratio(runs[0], ref, bound)
    print('%dx%d nsrc=%d %s: k_lag_gram worst err / bound %.4f' % (nz, nx, nsrc, fmt, worst))
    assert worst <= 1.0
    if fmt == 'complex128':          # bad arguments are refused before anything is launched
        f = helm_lib.helm_lag_gram_accumulate_device
        assert f(op.handle, P(dU.data_ptr()), nsrc, N - 1, d_c) == -1 and f(op.handle, P(dU.data_ptr()), 0, ld, d_c) == -1
        assert f(op.handle, None, nsrc, ld, d_c) == -1 and f(op.handle, P(dU.data_ptr()), nsrc, ld, None) == -1
        assert f(op.handle, P(dU.data_ptr() + 8), nsrc, ld, d_c) == -1 and f(op.handle, P(dU.data_ptr()), nsrc, ld, P(d_c.value + 8)) == -1
        assert f(op.handle, P(dU.data_ptr()), nsrc, ld, P(dU.data_ptr() + 16)) == -1
    else:          # no field, no exponents, values off 8 bytes, exponents off 4, ld < N, the output inside the field
        f, u, e = helm_lib.helm_lag_gram_accumulate_c64_device, dU.data_ptr(), dE.data_ptr()
        assert f(op.handle, None, P(e), nsrc, ld, d_c) == -1 and f(op.handle, P(u), None, nsrc, ld, d_c) == -1
        assert f(op.handle, P(u + 4), P(e), nsrc, ld, d_c) == -1 and f(op.handle, P(u), P(e + 2), nsrc, ld, d_c) == -1
        assert f(op.handle, P(u), P(e), nsrc, N - 1, d_c) == -1 and f(op.handle, P(u), P(e), nsrc, ld, P(u + 16)) == -1
    op.close()


def test_lag_gram_refuses_other_operators(helm_lib):
    import torch
    from zephyr_amd import _lib
    dev = torch.device('cuda', 0)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    Ne = int(helm_lib.helm_num_points(eu))
    ue, ce, he = (torch.zeros(n, dtype=t, device=dev) for n, t in ((Ne, torch.complex128), (13 * Ne, torch.complex128), (Ne, torch.float64)))
    torch.cuda.synchronize(dev)
    assert helm_lib.helm_lag_gram_accumulate_device(eu, P(ue.data_ptr()), 1, Ne, P(ce.data_ptr())) == -4          # (HELM_ERR_UNSUPPORTED)
    assert helm_lib.helm_gauss_newton_diagonal_device(eu, 0, None, None, P(ce.data_ptr()), P(ce.data_ptr()), 1.0, P(he.data_ptr())) == -4
    helm_lib.helm_destroy(eu)


# ---- 2. k_gauss_newton_diagonal -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', sorted(gc.GN_MODES))
@pytest.mark.parametrize('name', pc.HANDLES)
def test_combine_kernel_against_the_80_bit_evaluation(helm_lib, name, mode):
    """H += alpha W Re tr(E^H Gamma E Phi) on the four assembled handles of density_cases.OPERATOR_CASES in every mode, per cell within C_GN 2^-53
    (|H0| + alpha W M).  The planes are lag products of random columns, conjugated as the stored fields are; the entries k_lag_gram never writes hold NaN, so a
    read of one would show.  H starts non-zero between guard words, W and the chain are given and NULL, two runs give the same bits."""
    import torch
    lin, par, density = gc.GN_MODES[mode]
    sc, op, _ = pc.operator(name, 'explicit' if density else 'gardner', device=0)
    chain = None if density else fr.gardnerChain(sc['c'])
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
    Wh = rng.uniform(0.5, 2.0, N)
    dW = torch.from_numpy(Wh).to(dev)
    dChain = None if chain is None else torch.from_numpy(np.ascontiguousarray(chain)).to(dev)
    alpha = 0.37
    worst = {}
    for label, Wd, Wv in (('W', dW, Wh), ('noW', None, None)):
        ref0, mag0 = gc.combine_reference(op, Cu, Cg, mode, chain, alpha, Wv, np.zeros(N))
        H0 = rng.uniform(0.0, 1.0, N) * np.asarray(mag0, dtype=np.float64)
        H0[::3] = 0.0
        ref, mag = ref0 + H0.astype(LD), mag0 + H0.astype(LD)
        runs = []
        for rep in range(2):
            buf = torch.full((2 * GUARD + N,), 7.25, dtype=torch.float64, device=dev)
            buf[GUARD:GUARD + N] = torch.from_numpy(H0).to(dev)
            torch.cuda.synchronize(dev)
            op.gaussNewtonDiagonalDevice(mode, None if dChain is None else dChain.data_ptr(), None if Wd is None else Wd.data_ptr(), stored[0].data_ptr(),
                                         stored[1].data_ptr(), alpha, buf.data_ptr() + 8 * GUARD)
            h = buf.cpu().numpy()
            assert np.all(h[:GUARD] == 7.25) and np.all(h[GUARD + N:] == 7.25)
            runs.append(h[GUARD:GUARD + N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        assert np.all(np.isfinite(runs[0])) and np.any(runs[0] > H0)
        worst[label] = gc.worst_ratio(runs[0], ref, gc.C_GN * U64 * mag)
    print('%s %s: k_gauss_newton_diagonal worst err / bound %s' % (name, mode, ', '.join('%s %.4f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    del op.factors


def test_combine_kernel_refuses_bad_arguments(helm_lib):
    import torch
    from zephyr_amd import _lib
    sc, op, _ = pc.operator('even', 'explicit', device=0)
    N = 16
    dev = torch.device('cuda', 0)
    dCu, dCg = (torch.zeros(13 * N + 2, dtype=torch.complex128, device=dev) for _ in range(2))
    dW, dH, dC = (torch.zeros(N + 2, dtype=torch.float64, device=dev) for _ in range(3))
    torch.cuda.synchronize(dev)
    h, cu, cg, w, e, c = op.handle, dCu.data_ptr(), dCg.data_ptr(), dW.data_ptr(), dH.data_ptr(), dC.data_ptr()
    f = helm_lib.helm_gauss_newton_diagonal_device
    for mode in range(5):
        assert f(h, mode, P(c) if mode == 2 else None, P(w), P(cu), P(cg), 1.0, P(e)) == 0
    for bad in ((None, 0, None, P(w), P(cu), P(cg), 1.0, P(e)), (h, 0, None, P(w), None, P(cg), 1.0, P(e)), (h, 0, None, P(w), P(cu), None, 1.0, P(e)),
                (h, 0, None, P(w), P(cu), P(cg), 1.0, None), (h, 5, None, P(w), P(cu), P(cg), 1.0, P(e)), (h, -1, None, P(w), P(cu), P(cg), 1.0, P(e)),
                (h, 2, None, P(w), P(cu), P(cg), 1.0, P(e)), (h, 0, P(c), P(w), P(cu), P(cg), 1.0, P(e)), (h, 4, P(c), P(w), P(cu), P(cg), 1.0, P(e)),
                (h, 0, None, P(w), P(cu), P(cg), -1.0, P(e)), (h, 0, None, P(w), P(cu), P(cg), math.nan, P(e)), (h, 0, None, P(w + 4), P(cu), P(cg), 1.0, P(e)),
                (h, 0, None, P(w), P(cu + 8), P(cg), 1.0, P(e)), (h, 0, None, P(w), P(cu), P(cg + 8), 1.0, P(e)), (h, 0, None, P(w), P(cu), P(cg), 1.0, P(e + 4)),
                (h, 0, None, P(e), P(cu), P(cg), 1.0, P(e)), (h, 0, None, P(w), P(cu), P(cg), 1.0, P(cu)), (h, 2, P(e + 8), P(w), P(cu), P(cg), 1.0, P(e))):
        assert f(*bad) == -1, bad
    assert np.all(dH.cpu().numpy() == 0.0)                                      # (the planes were zero, and a refused call launches nothing)
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert raw, _lib.last_error(None)
    big = torch.zeros(13 * 108, dtype=torch.complex128, device=dev)
    hh = torch.zeros(108, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert f(raw, 0, None, None, P(big.data_ptr()), P(big.data_ptr()), 1.0, P(hh.data_ptr())) == -3          # (no assembled operator: HELM_ERR_STATE)
    helm_lib.helm_destroy(raw)
    del op.factors


# ---- 3. the routes --------------------------------------------------------------------------------------------------------------------------------------------
ROUTES = [('full_rho_given', False, 'complex128'), ('full_gardner', True, 'complex128'), ('full_rho_given', True, 'complex64'), ('full_gardner', False, 'complex64'),
          ('operator_rho', True, 'complex128'), ('operator_c', False, 'complex64'), ('scaler', True, 'complex128')]
EIGHT = [0, 3, 10, 12, 17, 21, 27, 33]          # of gaussnewton_cases.cells_37x53: a corner, a boundary line, beside it, under the free surface, two layers, the interior


def maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


@pytest.mark.parametrize('variant,hd,fmt', ROUTES, ids=['%s-%s-%s' % (v, 'hd' if h else 'mz', f) for v, h, f in ROUTES])
def test_routes_against_the_host_route_and_against_hvec(helm_lib, monkeypatch, variant, hd, fmt):
    """illumination(u=F, kind='gaussNewton') on the 37 x 53 pair with a fixed array, explicit and Gardner density, MiniZephyr and MiniZephyrHD (a complex
    scaleTerm), both stores: within 1e-6 in the max-norm of the host route fed the downloaded fields (the route tolerance of test_gpu_full.py: the receiver
    columns are solved twice, to solver accuracy), perFreq rows that sum to the total, the same bits twice and (complex128 store) from u = None, and within the
    same 1e-6 of e_i . Hvec(e_i, u=F) on the device at eight cells."""
    lin, par, density = gc.VARIANTS[variant]
    kw = dict(kind='gaussNewton', linearisation=lin, parameter=par)
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', hd, density=density, device=True, rtol=1e-11, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    D = prob.illumination(u=F, **kw)
    assert D.shape == (prob.nrow,) and D.dtype == np.float64 and np.all(D >= 0) and D.max() > 0
    host = prob.illumination(u=[F[f] for f in range(sv.nfreq)], **kw)
    e_host = maxrel(D, host)
    rows = prob.illumination(u=F, perFreq=True, **kw)
    assert rows.shape == (sv.nfreq, prob.nrow) and maxrel(rows.sum(axis=0), D) <= 1e-14
    assert np.array_equal(bits(prob.illumination(u=F, **kw)), bits(D))                                   # the same bits on every run
    if fmt == 'complex128':
        assert np.array_equal(bits(prob.illumination(**kw)), bits(D))                                    # solved into HBM, read and dropped
    cells = [gc.cells_37x53()[k] for k in EIGHT]
    want = gc.hvec_diagonal(prob, F, cells, linearisation=lin, parameter=par)
    e_hvec = maxrel(D[cells], want)
    print('%s hd=%s %s: |device - host| / max %.2e, |D[i] - e_i.Hvec(e_i)| / max %.2e, per cell %s' % (
        variant, hd, fmt, e_host, e_hvec, ' '.join('%.1e' % (abs(a - b) / abs(b)) if b else '0' for a, b in zip(D[cells], want))))
    assert e_host <= 1e-6 and e_hvec <= 1e-6
    if lin != 'scaler':
        assert ac.rel(prob.illumination(u=F, linearisation=lin, parameter=par), D) > 1e-3               # (not the pseudo-Hessian)
    F.release()
    del prob.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: every worker makes its own Gamma_f, the partials are added on the host"
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    kw = dict(kind='gaussNewton', linearisation='full')
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = xc.fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[xc.fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    host = prob.illumination(u=[F[0]], **kw)
    for H in (prob.illumination(u=F, **kw), prob.illumination(**kw)):
        assert maxrel(H, host) <= 1e-6
    F.release()
    del prob.factors


def test_refusals_on_the_device_path(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('relative', False, device=True)
    with pytest.raises(ValueError, match='fixed receiver arrays'):
        prob.illumination(kind='gaussNewton')
    prob, sv = xc.pair('fixed', False, device=True)
    with pytest.raises(ValueError, match='side'):
        prob.illumination(kind='gaussNewton', side='receiver')
    with pytest.raises(ValueError, match='gaussNewton'):
        prob.illumination(kind='gaussnewton')
