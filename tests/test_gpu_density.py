"""GPU: parameter='rho' on the device -- the four kernels of the density derivative through their C entry points against the 80-bit evaluations of
tests/density_cases.py under its componentwise bounds (every shape at which a walk takes another path, both store formats, ld > N, non-zero P / G, two runs
the same bits), the device routes of JvecBorn / Jtvec / Hvec against the host route on the oracle doubles, the Taylor test of dpred in rho through the device
routes, and the adjoint identities."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc, inner = ac.rel, ac.randc, ac.inner
OP = dict(linearisation='operator')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class RawHandle(object):
    'a library handle of a grid, created and never assembled: the two field kernels read the grid and the stream of a handle, not its operator'

    def __init__(self, lib, variant, nz, nx):
        from zephyr_amd import _lib
        self.lib, self.device = lib, 0
        self.handle = lib.helm_create(0, variant, nz, nx, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
        assert self.handle, _lib.last_error(None)

    def close(self):
        self.lib.helm_destroy(self.handle)


# ---- 1. k_stencil_sources and k_lag_imaging ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('case', dc.KERNEL_CASES, ids=['%dx%dx%d' % c for c in dc.KERNEL_CASES])
def test_field_kernels_against_the_80_bit_evaluation(helm_lib, case, fmt):
    """R = coef sum_k C_k shift_k(conj-or-not(U)) and P_k += sum_s UB_s shift_k(UF_s) per component within c 2^-53 of the magnitude sums of density_cases
    (c = 21 and 2 nsrc + 5, counted there from the kernels' operation order), plus 2^-24 of the same magnitude for the complex64 store.  Leading dimensions
    > N; guard cells, the gaps between columns and the boundary lines of P stay as they were; P starts non-zero; two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference
    nz, nx, nsrc = case
    op = RawHandle(helm_lib, _lib.HELM_MINIZEPHYR, nz, nx)
    dev = torch.device('cuda', op.device)
    N = nz * nx
    ldu, ldr, ldb, guard = N + 38, N + 11, N + 5, 517
    U, B, C, P0 = dc.kernel_inputs(nz, nx, nsrc, seed=100 * nz + nx + nsrc)
    coef = 0.3 - 1.1j
    fterm = 2.0 ** -24 if fmt == 'complex64' else 0.0
    Bpad = np.zeros((nsrc, ldb), dtype=np.complex128)
    Bpad[:, :N] = B
    dB, dC = torch.from_numpy(Bpad).to(dev), torch.from_numpy(C).to(dev)
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
                _lib.check(helm_lib.helm_stencil_sources_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), nsrc, ldu, P(dC.data_ptr()), coef.real, coef.imag,
                                                                    conj, d_r, ldr), op.handle)
            else:
                _lib.check(helm_lib.helm_stencil_sources_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dC.data_ptr()), coef.real, coef.imag, conj, d_r, ldr), op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + nsrc * ldr:] == fill)
            body = h[guard:guard + nsrc * ldr].reshape((nsrc, ldr))
            assert np.all(body[:, N:] == fill)
            runs.append(body[:, :N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = dc.stencil_sources_reference(U, C, coef, nz, nx, bool(conj))
        worst['stencil conj=%d' % conj] = dc.worst_ratio(runs[0], ref, (dc.C_STENCIL * dc.U64 + fterm) * mag)
    runs = []
    for _ in range(2):
        buf = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
        buf[guard:guard + 9 * N] = torch.from_numpy(P0.ravel()).to(dev)
        torch.cuda.synchronize(dev)
        d_p = P(buf.data_ptr() + 16 * guard)
        if fmt == 'complex64':
            _lib.check(helm_lib.helm_lag_imaging_accumulate_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, d_p), op.handle)
        else:
            _lib.check(helm_lib.helm_lag_imaging_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, d_p), op.handle)
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
        runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    ref, mag = dc.lag_imaging_reference(P0, U, B, nz, nx)
    worst['lag'] = dc.worst_ratio(runs[0], ref, (dc.c_lag(nsrc) * dc.U64 + fterm) * mag)
    edge = ~np.asarray(dc.fr._interiorMask(nz, nx)).ravel()
    assert np.array_equal(bits(runs[0][:, edge]), bits(P0[:, edge]))                    # (the boundary lines of P are not written)
    print('%dx%d nsrc=%d %s: worst err / bound %s' % (nz, nx, nsrc, fmt, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(w <= 1.0 for w in worst.values()), worst
    if fmt == 'complex128':          # bad arguments are refused before anything is launched
        assert helm_lib.helm_stencil_sources_device(op.handle, P(dU.data_ptr()), nsrc, N - 1, P(dC.data_ptr()), 1.0, 0.0, 0, d_r, ldr) == -1
        assert helm_lib.helm_stencil_sources_device(op.handle, P(dU.data_ptr()), 0, ldu, P(dC.data_ptr()), 1.0, 0.0, 0, d_r, ldr) == -1
        assert helm_lib.helm_stencil_sources_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dC.data_ptr()), 1.0, 0.0, 0, P(d_r.value + 8), ldr) == -1
        assert helm_lib.helm_stencil_sources_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dC.data_ptr()), 1.0, 0.0, 0, P(dC.data_ptr() + 16), N) == -1
        assert helm_lib.helm_lag_imaging_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), N - 1, nsrc, d_p) == -1
        assert helm_lib.helm_lag_imaging_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, P(dB.data_ptr())) == -1
    else:          # the complex64 halves: no field, no exponents, values off 8 bytes, exponents off 4, ld < N, the output inside the field
        u, e, c, b = dU.data_ptr(), dE.data_ptr(), P(dC.data_ptr()), P(dB.data_ptr())
        st, lg = helm_lib.helm_stencil_sources_c64_device, helm_lib.helm_lag_imaging_accumulate_c64_device
        for pu, pe, l, r in ((None, P(e), ldu, d_r), (P(u), None, ldu, d_r), (P(u + 4), P(e), ldu, d_r), (P(u), P(e + 2), ldu, d_r), (P(u), P(e), N - 1, d_r),
                             (P(u), P(e), ldu, P(u + 16))):
            assert st(op.handle, pu, pe, nsrc, l, c, 1.0, 0.0, 0, r, ldr) == -1
        for pu, pe, l, p in ((None, P(e), ldu, d_p), (P(u), None, ldu, d_p), (P(u + 4), P(e), ldu, d_p), (P(u), P(e + 2), ldu, d_p), (P(u), P(e), N - 1, d_p),
                             (P(u), P(e), ldu, P(u + 16))):
            assert lg(op.handle, pu, pe, l, b, ldb, nsrc, p) == -1
    op.close()


# ---- 2. k_buoyancy_planes and k_buoyancy_adjoint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_buoyancy_kernels_against_the_80_bit_evaluation(helm_lib, name):
    """dC = L[db] and G += w (conj-or-not L)^T P on assembled handles (free-surface flags on and off, dx != dz, ky, a damped frequency) per component within
    C_PLANES = 48 and C_ADJOINT = 67 times 2^-53 of the magnitudes of density_cases; guard cells stay, G starts non-zero, two runs give the same bits."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = dc.operator_config(name)
    op = za.MiniZephyr(dict(sc, device=0))
    db, Pl, G0 = dc.operator_inputs(sc)
    N = db.size
    dev = torch.device('cuda', 0)
    guard, fill = 517, complex(7.0, -3.0)
    dDb, dP = torch.from_numpy(db).to(dev), torch.from_numpy(Pl).to(dev)
    runs = []
    for _ in range(2):
        out = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
        torch.cuda.synchronize(dev)
        d_c = P(out.data_ptr() + 16 * guard)
        _lib.check(helm_lib.helm_buoyancy_planes_device(op.handle, P(dDb.data_ptr()), d_c), op.handle)
        h = out.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
        runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    edge = ~np.asarray(dc.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    assert np.all(runs[0][:, edge] == 0)
    ref, mag = dc.planes_reference(op, db)
    worst = {'planes': dc.worst_ratio(runs[0], ref, dc.C_PLANES * dc.U64 * mag)}
    w = -0.7 + 0.4j
    for conj in (0, 1):
        runs = []
        for _ in range(2):
            buf = torch.full((2 * guard + N,), fill, dtype=torch.complex128, device=dev)
            buf[guard:guard + N] = torch.from_numpy(G0).to(dev)
            torch.cuda.synchronize(dev)
            d_g = P(buf.data_ptr() + 16 * guard)
            _lib.check(helm_lib.helm_buoyancy_adjoint_device(op.handle, P(dP.data_ptr()), w.real, w.imag, conj, d_g), op.handle)
            h = buf.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + N:] == fill)
            runs.append(h[guard:guard + N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = dc.adjoint_reference(op, G0, Pl, w, bool(conj))
        worst['adjoint conj=%d' % conj] = dc.worst_ratio(runs[0], ref, dc.C_ADJOINT * dc.U64 * mag)
    print('%s: worst err / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    assert helm_lib.helm_buoyancy_planes_device(op.handle, P(dDb.data_ptr() + 4), d_c) == -1
    assert helm_lib.helm_buoyancy_adjoint_device(op.handle, P(dP.data_ptr()), 1.0, 0.0, 0, P(dP.data_ptr() + 16)) == -1
    del op.factors


def test_unassembled_eurus_and_3d_handles_are_refused(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    raw = RawHandle(helm_lib, _lib.HELM_MINIZEPHYR, 12, 9)
    a, b = torch.zeros(9 * 108, dtype=torch.complex128, device='cuda'), torch.zeros(108, dtype=torch.complex128, device='cuda')
    d = torch.zeros(108, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert helm_lib.helm_buoyancy_planes_device(raw.handle, P(d.data_ptr()), P(a.data_ptr())) == -3          # (no assembled operator: HELM_ERR_STATE)
    assert helm_lib.helm_buoyancy_adjoint_device(raw.handle, P(a.data_ptr()), 1.0, 0.0, 0, P(b.data_ptr())) == -3
    raw.close()
    eu = RawHandle(helm_lib, _lib.HELM_EURUS, 36, 40)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for o in (eu, h3):
        N = int(helm_lib.helm_num_points(o.handle))
        u, r, g = [torch.zeros(N, dtype=torch.complex128, device='cuda') for _ in range(3)]
        c = torch.zeros(9 * N, dtype=torch.complex128, device='cuda')
        d = torch.zeros(N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        assert helm_lib.helm_buoyancy_planes_device(o.handle, P(d.data_ptr()), P(c.data_ptr())) == -4
        assert helm_lib.helm_stencil_sources_device(o.handle, P(u.data_ptr()), 1, N, P(c.data_ptr()), 1.0, 0.0, 0, P(r.data_ptr()), N) == -4
        assert helm_lib.helm_lag_imaging_accumulate_device(o.handle, P(u.data_ptr()), N, P(r.data_ptr()), N, 1, P(c.data_ptr())) == -4
        assert helm_lib.helm_buoyancy_adjoint_device(o.handle, P(c.data_ptr()), 1.0, 0.0, 0, P(g.data_ptr())) == -4
    eu.close()
    del h3.factors


# ---- 3. the device routes against the host route ---------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm


@pytest.fixture(scope='module')
def host_ref():
    'per mode, from the oracle doubles on the host route, made once: a density perturbation, a residual and the operator products'
    out = {}
    for mode, hd in E2E.items():
        probh, svh = fc.host_pair(mode, hd)
        rng = np.random.default_rng(31)
        v, p, r = dc.perturbation(), rng.standard_normal(probh.nrow), randc(rng, svh.nD)
        uF = probh.fields()
        kw = dict(u=uF, **OP)
        out[mode] = dict(prob=probh, sv=svh, v=v, p=p, r=r, Jv=probh.JvecBorn(None, v, parameter='rho', **kw),
                         gT=probh.Jtvec(None, r, adjoint='transpose', parameter='rho', **kw), Hv=probh.Hvec(None, v, parameter='rho', **kw),
                         Hx=probh.Hvec(None, p, parameter=('c', 'rho'), **kw))
    return out


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_route_with_the_store_and_without(helm_lib, monkeypatch, host_ref, mode):
    """complex128 store: the tolerance 1e-6 and the identity at 1e-7 are those of the 'operator' device-against-host tests of test_gpu_frechet.py (the solver
    runs at rtol 1e-11 against the oracle's LU); u = None gives the same bits as u = F; Jtvec twice gives the same bits."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, p, r = h['v'], h['p'], h['r']
    prob, sv = fc.device_pair(mode, E2E[mode], rtol=1e-11)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    kw = dict(u=F, **OP)
    gT, Jv = prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **kw), prob.JvecBorn(None, v, parameter='rho', **kw)
    Hv, Hx = prob.Hvec(None, v, parameter='rho', **kw), prob.Hvec(None, p, parameter=('c', 'rho'), **kw)
    assert gT.shape == (prob.nrow,) and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128 and Hv.dtype == np.float64
    eg, ej, eh, ex = rel(gT, h['gT']), rel(Jv, h['Jv']), rel(Hv, h['Hv']), rel(Hx, h['Hx'])
    lhs = inner(Jv, r)
    miss = abs(lhs - inner(v, gT)) / abs(lhs)
    print('%s: Jtvec against the host route %.2e, JvecBorn %.2e, Hvec %.2e, Hvec (c, rho) %.2e; identity misses by %.2e' % (mode, eg, ej, eh, ex, miss))
    assert eg <= 1e-6 and ej <= 1e-6 and eh <= 1e-6 and ex <= 1e-6
    assert miss <= 1e-7
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **kw)), bits(gT))          # (twice: the same bits)
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', parameter='rho', **OP)), bits(gT))          # (u = None: the same launches)
    assert np.array_equal(bits(prob.JvecBorn(None, v, parameter='rho', **OP)), bits(Jv))
    assert rel(prob.Hvec(None, v, parameter='rho', **OP), Hv) <= 1e-12
    # the off-diagonal blocks are each other's transposes
    a, b = float(v @ Hx), float(p @ prob.Hvec(None, v, parameter=('rho', 'c'), **kw))
    assert abs(a - b) <= 1e-7 * max(abs(a), abs(b))
    # parameter='c' is the route as it was
    assert np.array_equal(bits(prob.JvecBorn(None, p, parameter='c', **kw)), bits(prob.JvecBorn(None, p, **kw)))
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', parameter='c', **kw)), bits(prob.Jtvec(None, r, adjoint='transpose', **kw)))
    with pytest.raises(ValueError):
        prob.JvecBorn(None, v, u=F, parameter='rho')
    F.release()
    del prob.factors


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_complex64_store_against_the_host_route_on_the_unpacked_fields(helm_lib, monkeypatch, host_ref, mode):
    "the format bound of test_gpu_frechet.py's complex64 test: the device on the packed store against the host route on the same, unpacked fields"
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, r, probh = h['v'], h['r'], h['prob']
    prob64, sv64 = fc.device_pair(mode, E2E[mode], rtol=1e-11, fieldsDtype='complex64')
    F64 = prob64.fieldsDevice()
    assert F64.dtype == 'complex64'
    kw = dict(u=F64, parameter='rho', **OP)
    d64, g64 = prob64.JvecBorn(None, v, **kw), prob64.Jtvec(None, r, adjoint='transpose', **kw)
    unpacked = list(F64)
    dh = probh.JvecBorn(None, v, u=unpacked, parameter='rho', **OP)
    gh = probh.Jtvec(None, r, u=unpacked, adjoint='transpose', parameter='rho', **OP)
    print('%s complex64: JvecBorn against the host route on the unpacked fields %.2e, Jtvec %.2e' % (mode, rel(d64, dh), rel(g64, gh)))
    assert rel(d64, dh) <= 1e-6 and rel(g64, gh) <= 1e-6
    assert rel(d64, h['Jv']) > 0                                       # (the packed store was read)
    lhs = inner(d64, r)
    assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    F64.release()
    del prob64.factors


# ---- 4. Taylor through the device routes -----------------------------------------------------------------------------------------------------------
def test_taylor_remainder_of_the_device_dpred_in_rho_falls_at_second_order(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = fc.device_pair('fixed', False, rtol=1e-11)
    rho0 = np.array(prob.systemConfig['rho'], dtype=np.float64)
    v = dc.perturbation()
    F = prob.fieldsDevice()
    Jv = prob.JvecBorn(None, v, u=F, parameter='rho', **OP)
    F.release()
    r = dc.taylor_remainders(sv, Jv, rho0, v)
    print('device: remainders %s factors %s' % (r, fc.factors(r)))
    assert all(f >= 3.5 for f in fc.factors(r))
    del prob.factors
