"""GPU: linearisation='operator' on the device -- k_virtual_sources_op / k_imaging_op against the 80-bit evaluation of tests/frechet_cases.py under its
componentwise bound (every shape at which the walk takes another path, both store formats, ld > N, two runs the same bits), the device routes of JvecBorn /
Jtvec / Hvec against the host route on the oracle doubles, the Taylor test of dpred once through the device routes, and the symmetry of Hvec."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import frechet_cases as fc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc, inner = ac.rel, ac.randc, ac.inner


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 6. the two kernels --------------------------------------------------------------------------------------------------------------------------
# 12 x 9: every cell is next to a boundary line; 3 x 70: a single interior row, two tiles along x; 5 x 300: dx != dz, five tiles, the rolling window at its
# minimum of three interior rows; 37 x 53: no multiple of the wave, two row chunks.  nsrc 1 and 3 are below the four columns walked together, 13 is three
# groups and a remainder of one.
SHAPES = {(12, 9): (10., 10.), (3, 70): (10., 10.), (5, 300): (10., 7.), (37, 53): (12.5, 12.5)}


class RawHandle(object):
    'a library handle of a grid, created and never assembled: the two kernels read the grid and the stream of a handle, not its operator'

    def __init__(self, lib, variant, nz, nx, dx, dz):
        from zephyr_amd import _lib
        self.lib, self.device = lib, 0
        self.handle = lib.helm_create(0, variant, nz, nx, float(dx), float(dz), 2, (ctypes.c_int * 4)(0, 0, 0, 0))
        assert self.handle, _lib.last_error(None)

    def close(self):
        self.lib.helm_destroy(self.handle)


@pytest.fixture(scope='module')
def handles(helm_lib):
    from zephyr_amd import _lib
    ops = {s: RawHandle(helm_lib, _lib.HELM_MINIZEPHYR, s[0], s[1], d[0], d[1]) for s, d in SHAPES.items()}
    yield ops
    for o in ops.values():
        o.close()


@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('nsrc', [1, 3, 13])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_both_kernels_against_the_80_bit_evaluation(helm_lib, handles, shape, nsrc, fmt):
    """R = coef mask_int M0(W conj-or-not(U)) and G += W sum_s UF_s M0(mask_int UB_s) per component within c 2^-53 times the magnitude sums of
    frechet_cases (c = 12 for the virtual sources, 13 + nsrc for the imaging sum, counted there from the kernels' operation order); the complex64 store adds
    the format term 2^-24 of the same magnitude (every stored component is within 2^-24 relative of the packed one).  Leading dimensions > N, guard cells and
    the gaps between columns stay as they were, two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference
    nz, nx = shape
    op = handles[shape]
    dev = torch.device('cuda', op.device)
    N = nz * nx
    ldu, ldr, ldb, guard = N + 38, N + 11, N + 5, 517
    U, B, W, G0 = fc.kernel_inputs(nz, nx, nsrc, seed=100 * nz + nsrc)
    coef = 0.3 - 1.1j
    fterm = 2.0 ** -24 if fmt == 'complex64' else 0.0
    Bpad = np.zeros((nsrc, ldb), dtype=np.complex128)
    Bpad[:, :N] = B
    dB, dW = torch.from_numpy(Bpad).to(dev), torch.from_numpy(W).to(dev)
    if fmt == 'complex64':
        Pk, e = pack_reference(np.ascontiguousarray(U.T))
        Ppad = np.zeros((nsrc, ldu), dtype=np.complex64)
        Ppad[:, :N] = Pk.T
        dU, dE = torch.from_numpy(Ppad).to(dev), torch.from_numpy(e).to(dev)
    else:
        Upad = np.zeros((nsrc, ldu), dtype=np.complex128)
        Upad[:, :N] = U
        dU, dE = torch.from_numpy(Upad).to(dev), None
    fill = complex(7.0, -3.0)
    worst = {}
    for conj in (0, 1):
        runs = []
        for _ in range(2):
            out = torch.full((2 * guard + nsrc * ldr,), fill, dtype=torch.complex128, device=dev)
            torch.cuda.synchronize(dev)
            d_r = P(out.data_ptr() + 16 * guard)
            if fmt == 'complex64':
                _lib.check(helm_lib.helm_virtual_sources_op_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), nsrc, ldu, P(dW.data_ptr()), coef.real, coef.imag,
                                                                       conj, d_r, ldr), op.handle)
            else:
                _lib.check(helm_lib.helm_virtual_sources_op_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dW.data_ptr()), coef.real, coef.imag, conj, d_r, ldr),
                           op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + nsrc * ldr:] == fill)
            body = h[guard:guard + nsrc * ldr].reshape((nsrc, ldr))
            assert np.all(body[:, N:] == fill)
            runs.append(body[:, :N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = fc.virtual_sources_reference(U, W, coef, nz, nx, bool(conj))
        worst['virtual conj=%d' % conj] = fc.worst_ratio(runs[0], ref, (fc.C_VIRTUAL * fc.U64 + fterm) * mag)
    runs = []
    for _ in range(2):
        buf = torch.full((2 * guard + N,), fill, dtype=torch.complex128, device=dev)
        buf[guard:guard + N] = torch.from_numpy(G0).to(dev)
        torch.cuda.synchronize(dev)
        d_g = P(buf.data_ptr() + 16 * guard)
        if fmt == 'complex64':
            _lib.check(helm_lib.helm_imaging_op_accumulate_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, P(dW.data_ptr()), d_g),
                       op.handle)
        else:
            _lib.check(helm_lib.helm_imaging_op_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, P(dW.data_ptr()), d_g), op.handle)
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + N:] == fill)
        runs.append(h[guard:guard + N].copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    ref, mag = fc.imaging_reference(G0, U, B, W, nz, nx)
    worst['imaging'] = fc.worst_ratio(runs[0], ref, (fc.c_imaging(nsrc) * fc.U64 + fterm) * mag)
    print('%dx%d nsrc=%d %s: worst err / bound %s' % (nz, nx, nsrc, fmt, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(w <= 1.0 for w in worst.values()), worst
    # bad arguments are refused before anything is launched
    if fmt == 'complex128':
        assert helm_lib.helm_virtual_sources_op_device(op.handle, P(dU.data_ptr()), nsrc, N - 1, P(dW.data_ptr()), 1.0, 0.0, 0, d_r, ldr) == -1
        assert helm_lib.helm_virtual_sources_op_device(op.handle, P(dU.data_ptr()), 0, ldu, P(dW.data_ptr()), 1.0, 0.0, 0, d_r, ldr) == -1
        assert helm_lib.helm_virtual_sources_op_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dW.data_ptr()), 1.0, 0.0, 0, P(d_r.value + 8), ldr) == -1
        assert helm_lib.helm_imaging_op_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), N - 1, nsrc, P(dW.data_ptr()), d_g) == -1
        assert helm_lib.helm_imaging_op_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, P(dW.data_ptr()), P(dW.data_ptr())) == -1
    else:          # the complex64 halves: no field, no exponents, values off 8 bytes, exponents off 4, ld < N, the output on the field
        u, e, w, b = dU.data_ptr(), dE.data_ptr(), P(dW.data_ptr()), P(dB.data_ptr())
        vs, im = helm_lib.helm_virtual_sources_op_c64_device, helm_lib.helm_imaging_op_accumulate_c64_device
        for pu, pe, l, r in ((None, P(e), ldu, d_r), (P(u), None, ldu, d_r), (P(u + 4), P(e), ldu, d_r), (P(u), P(e + 2), ldu, d_r), (P(u), P(e), N - 1, d_r),
                             (P(u), P(e), ldu, P(u))):
            assert vs(op.handle, pu, pe, nsrc, l, w, 1.0, 0.0, 0, r, ldr) == -1
        for pu, pe, l, g in ((None, P(e), ldu, d_g), (P(u), None, ldu, d_g), (P(u + 4), P(e), ldu, d_g), (P(u), P(e + 2), ldu, d_g), (P(u), P(e), N - 1, d_g),
                             (P(u), P(e), ldu, P(u))):
            assert im(op.handle, pu, pe, l, b, ldb, nsrc, w, g) == -1


def test_eurus_and_3d_handles_are_unsupported(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    eu = RawHandle(helm_lib, _lib.HELM_EURUS, 36, 40, 10., 10.)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for o in (eu, h3):
        N = int(helm_lib.helm_num_points(o.handle))
        assert N > 0
        a, b, w, g = [torch.zeros(N, dtype=torch.complex128, device='cuda') for _ in range(4)]
        torch.cuda.synchronize()
        assert helm_lib.helm_virtual_sources_op_device(o.handle, P(a.data_ptr()), 1, N, P(w.data_ptr()), 1.0, 0.0, 0, P(b.data_ptr()), N) == -4
        assert helm_lib.helm_imaging_op_accumulate_device(o.handle, P(a.data_ptr()), N, P(b.data_ptr()), N, 1, P(w.data_ptr()), P(g.data_ptr())) == -4
    eu.close()
    del h3.factors


# ---- 7. the device routes against the host route -------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm


@pytest.fixture(scope='module')
def host_ref():
    'per mode, from the oracle doubles on the host route, made once: fields, a model vector, a residual, and the three operator products'
    out = {}
    for mode, hd in E2E.items():
        probh, svh = fc.host_pair(mode, hd)
        rng = np.random.default_rng(31)
        v, r = rng.standard_normal(probh.nrow), randc(rng, svh.nD)
        uF = probh.fields()
        kw = dict(u=uF, linearisation='operator')
        out[mode] = dict(prob=probh, sv=svh, v=v, r=r, uF=uF, Jv=probh.JvecBorn(None, v, **kw), gT=probh.Jtvec(None, r, adjoint='transpose', **kw),
                         Hv=probh.Hvec(None, v, **kw))
    return out


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_route_with_the_store_and_without(helm_lib, monkeypatch, host_ref, mode):
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, r = h['v'], h['r']
    prob, sv = fc.device_pair(mode, E2E[mode], rtol=1e-11)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    kw = dict(u=F, linearisation='operator')
    gT, Jv, Hv = prob.Jtvec(None, r, adjoint='transpose', **kw), prob.JvecBorn(None, v, **kw), prob.Hvec(None, v, **kw)
    assert gT.shape == (prob.nrow,) and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128 and Hv.dtype == np.float64
    eg, ej, eh = rel(gT, h['gT']), rel(Jv, h['Jv']), rel(Hv, h['Hv'])
    lhs = inner(Jv, r)
    miss = abs(lhs - inner(v, gT)) / abs(lhs)
    print('%s: Jtvec against the host route %.2e, JvecBorn %.2e, Hvec %.2e; identity misses by %.2e' % (mode, eg, ej, eh, miss))
    assert eg <= 1e-6 and ej <= 1e-6 and eh <= 1e-6
    assert miss <= 1e-7
    # u = None: fieldsDevice inside, the same launches on the same inputs
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', linearisation='operator')), bits(gT))
    assert np.array_equal(bits(prob.JvecBorn(None, v, linearisation='operator')), bits(Jv))
    assert rel(prob.Hvec(None, v, linearisation='operator'), Hv) <= 1e-12
    # the default keyword is the route as it was
    assert np.array_equal(bits(prob.JvecBorn(None, v, u=F, linearisation='scaler')), bits(prob.JvecBorn(None, v, u=F)))
    assert np.array_equal(bits(prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='scaler')), bits(prob.Jtvec(None, r, u=F, adjoint='transpose')))
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=F, linearisation='operator')
    F.release()
    del prob.factors


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_complex64_store_against_the_host_route_on_the_unpacked_fields(helm_lib, monkeypatch, host_ref, mode):
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, r, probh = h['v'], h['r'], h['prob']
    prob64, sv64 = fc.device_pair(mode, E2E[mode], rtol=1e-11, fieldsDtype='complex64')
    F64 = prob64.fieldsDevice()
    assert F64.dtype == 'complex64'
    kw = dict(u=F64, linearisation='operator')
    d64, g64 = prob64.JvecBorn(None, v, **kw), prob64.Jtvec(None, r, adjoint='transpose', **kw)
    unpacked = list(F64)
    dh = probh.JvecBorn(None, v, u=unpacked, linearisation='operator')
    gh = probh.Jtvec(None, r, u=unpacked, adjoint='transpose', linearisation='operator')
    print('%s complex64: JvecBorn against the host route on the unpacked fields %.2e, Jtvec %.2e' % (mode, rel(d64, dh), rel(g64, gh)))
    assert rel(d64, dh) <= 1e-6 and rel(g64, gh) <= 1e-6
    assert rel(d64, h['Jv']) > 0                                       # (the packed store was read)
    lhs = inner(d64, r)
    assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    F64.release()
    del prob64.factors


# ---- 8. Taylor through the device routes -----------------------------------------------------------------------------------------------------------
def test_taylor_remainder_of_the_device_dpred_falls_at_second_order(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = fc.device_pair('fixed', False, rtol=1e-11)
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    v = fc.perturbation()
    F = prob.fieldsDevice(c0)
    Jop = prob.JvecBorn(None, v, u=F, linearisation='operator')
    Jsc = prob.JvecBorn(None, v, u=F)
    F.release()
    dpred = lambda c: sv.dpred(c)
    r_op, r_sc = fc.taylor_remainders(dpred, Jop, c0, v), fc.taylor_remainders(dpred, Jsc, c0, v)
    print('device: operator remainders %s factors %s; scaler factors %s' % (r_op, fc.factors(r_op), fc.factors(r_sc)))
    assert all(f >= 3.5 for f in fc.factors(r_op))
    assert all(f <= 2.5 for f in fc.factors(r_sc))
    del prob.factors


# ---- 9. Hvec is symmetric --------------------------------------------------------------------------------------------------------------------------
def test_hvec_with_the_operator_linearisation_is_symmetric(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = fc.device_pair('relative', True, rtol=1e-11)
    F = prob.fieldsDevice()
    rng = np.random.default_rng(37)
    p, q = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow)
    Hp, Hq = prob.Hvec(None, p, u=F, linearisation='operator'), prob.Hvec(None, q, u=F, linearisation='operator')
    a, b = float(p @ Hq), float(q @ Hp)
    print('Hvec symmetry: %.6e against %.6e' % (a, b))
    assert abs(a - b) <= 1e-7 * max(abs(a), abs(b))
    assert float(p @ Hp) > 0
    F.release()
    del prob.factors
