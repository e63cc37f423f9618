"""GPU: linearisation='full' on the device -- k_velocity_planes and k_velocity_adjoint through their C entry points against the 80-bit evaluations of
tests/full_cases.py under its componentwise bounds (dDb NULL and given, conj 0 and 1, a non-zero G, NaN boundary rows of P, two runs the same bits), the device
routes of JvecBorn / Jtvec / Hvec against the host route on the oracle doubles (both stores, fixed and moving arrays, u = F and u = None, with and without
`rho`), the Taylor test of dpred through the device routes, the adjoint identity, and the routes that must stay as they were against their recording."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc, inner = ac.rel, ac.randc, ac.inner
FULL = dict(linearisation='full')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. k_velocity_planes and k_velocity_adjoint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_velocity_kernels_against_the_80_bit_evaluation(helm_lib, name):
    """dC = V[dc] (+ L[db]) and G += w (conj-or-not V)^T P on assembled handles (3 x 3, 4 x 4, 5 x 63, 33 x 125: free-surface flags on and off, dx != dz, ky, a
    damped frequency) per component within C_VPLANES = 68 (69 with db) and C_VADJOINT = 98 times 2^-53 of the magnitudes of full_cases; guard cells stay, G
    starts non-zero, the boundary rows of P are NaN, two runs give the same bits."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = xc.operator_config(name)
    op = za.MiniZephyr(dict(sc, device=0))
    v, db, Pl, G0 = xc.operator_inputs(sc)
    N = v.size
    dev = torch.device('cuda', 0)
    guard, fill = 517, complex(7.0, -3.0)
    edge = ~np.asarray(dc.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    Pnan = Pl.copy()
    Pnan[:, edge] = complex(np.nan, np.nan)
    dDc, dDb, dP = torch.from_numpy(v).to(dev), torch.from_numpy(db).to(dev), torch.from_numpy(Pnan).to(dev)
    worst = {}
    for label, d_db, host_db, c in (('planes', None, None, xc.C_VPLANES), ('planes+db', P(dDb.data_ptr()), db, xc.C_VPLANES_DB)):
        runs = []
        for _ in range(2):
            out = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
            torch.cuda.synchronize(dev)
            d_c = P(out.data_ptr() + 16 * guard)
            _lib.check(helm_lib.helm_velocity_planes_device(op.handle, P(dDc.data_ptr()), d_db, d_c), op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
            runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        assert np.all(runs[0][:, edge] == 0)
        ref, mag = xc.planes_reference(op, v, host_db)
        worst[label] = xc.worst_ratio(runs[0], ref, c * xc.U64 * mag)
    w = -0.7 + 0.4j
    for conj in (0, 1):
        runs = []
        for _ in range(2):
            buf = torch.full((2 * guard + N,), fill, dtype=torch.complex128, device=dev)
            buf[guard:guard + N] = torch.from_numpy(G0).to(dev)
            torch.cuda.synchronize(dev)
            d_g = P(buf.data_ptr() + 16 * guard)
            _lib.check(helm_lib.helm_velocity_adjoint_device(op.handle, P(dP.data_ptr()), w.real, w.imag, conj, d_g), op.handle)
            h = buf.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + N:] == fill)
            runs.append(h[guard:guard + N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        assert np.all(np.isfinite(runs[0].view(np.float64)))                 # (the NaN boundary rows of P were not read)
        ref, mag = xc.adjoint_reference(op, G0, Pl, w, bool(conj))
        worst['adjoint conj=%d' % conj] = xc.worst_ratio(runs[0], ref, xc.C_VADJOINT * xc.U64 * mag)
        assert np.any(runs[0] != G0)
    print('%s: worst err / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    # bad arguments are refused before anything is launched
    assert helm_lib.helm_velocity_planes_device(op.handle, P(dDc.data_ptr() + 4), None, d_c) == -1
    assert helm_lib.helm_velocity_planes_device(op.handle, P(dDc.data_ptr()), P(dDb.data_ptr() + 4), d_c) == -1
    assert helm_lib.helm_velocity_planes_device(op.handle, None, None, d_c) == -1
    assert helm_lib.helm_velocity_planes_device(op.handle, P(dDc.data_ptr()), None, P(dDc.data_ptr())) == -1
    assert helm_lib.helm_velocity_adjoint_device(op.handle, P(dP.data_ptr()), 1.0, 0.0, 0, P(dP.data_ptr() + 16)) == -1
    assert helm_lib.helm_velocity_adjoint_device(op.handle, P(dP.data_ptr() + 8), 1.0, 0.0, 0, d_g) == -1
    del op.factors


def test_unassembled_eurus_and_3d_handles_are_refused(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert raw, _lib.last_error(None)
    a, b = torch.zeros(9 * 108, dtype=torch.complex128, device='cuda'), torch.zeros(108, dtype=torch.complex128, device='cuda')
    d = torch.zeros(108, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert helm_lib.helm_velocity_planes_device(raw, P(d.data_ptr()), None, P(a.data_ptr())) == -3          # (no assembled operator: HELM_ERR_STATE)
    assert helm_lib.helm_velocity_adjoint_device(raw, P(a.data_ptr()), 1.0, 0.0, 0, P(b.data_ptr())) == -3
    helm_lib.helm_destroy(raw)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for handle in (eu, h3.handle):
        N = int(helm_lib.helm_num_points(handle))
        g = torch.zeros(N, dtype=torch.complex128, device='cuda')
        c = torch.zeros(9 * N, dtype=torch.complex128, device='cuda')
        d = torch.zeros(N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        assert helm_lib.helm_velocity_planes_device(handle, P(d.data_ptr()), None, P(c.data_ptr())) == -4
        assert helm_lib.helm_velocity_adjoint_device(handle, P(c.data_ptr()), 1.0, 0.0, 0, P(g.data_ptr())) == -4
    helm_lib.helm_destroy(eu)
    del h3.factors


# ---- 2. the device routes against the host route ---------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm
ROUTES = [(mode, density) for mode in ('fixed', 'relative') for density in (True, False)]
ROUTE_IDS = ['%s-%s' % (m, 'rho' if d else 'gardner') for m, d in ROUTES]


@pytest.fixture(scope='module')
def host_ref():
    'per mode and density, from the oracle doubles on the host route, made once: a perturbation non-zero everywhere, a residual and the three products'
    out = {}
    for mode, density in ROUTES:
        probh, svh = xc.pair(mode, E2E[mode], density=density)
        rng = np.random.default_rng(31)
        v, p, r = xc.perturbation(), rng.standard_normal(probh.nrow), randc(rng, svh.nD)
        uF = probh.fields()
        kw = dict(u=uF, **FULL)
        out[(mode, density)] = dict(prob=probh, sv=svh, v=v, p=p, r=r, Jv=probh.JvecBorn(None, v, **kw), gT=probh.Jtvec(None, r, adjoint='transpose', **kw),
                                    Hp=probh.Hvec(None, p, **kw))
    return out


@pytest.mark.parametrize('mode,density', ROUTES, ids=ROUTE_IDS)
def test_device_routes_against_the_host_route_with_the_store_and_without(helm_lib, monkeypatch, host_ref, mode, density):
    """complex128 store: the tolerance 1e-6 and the identity at 1e-7 are those of the 'operator' device-against-host tests of test_gpu_frechet.py (the solver
    runs at rtol 1e-11 against the oracle's LU); u = None gives the same bits as u = F; two consecutive calls give the same bits."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[(mode, density)]
    v, p, r = h['v'], h['p'], h['r']
    prob, sv = xc.pair(mode, E2E[mode], density=density, device=True, rtol=1e-11)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    kw = dict(u=F, **FULL)
    gT, Jv, Hp = prob.Jtvec(None, r, adjoint='transpose', **kw), prob.JvecBorn(None, v, **kw), prob.Hvec(None, p, **kw)
    assert gT.shape == (prob.nrow,) and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128 and Hp.dtype == np.float64
    eg, ej, eh = rel(gT, h['gT']), rel(Jv, h['Jv']), rel(Hp, h['Hp'])
    lhs = inner(Jv, r)
    miss = abs(lhs - inner(v, gT)) / abs(lhs)
    print('%s %s: Jtvec against the host route %.2e, JvecBorn %.2e, Hvec %.2e; identity misses by %.2e' % (mode, density, eg, ej, eh, miss))
    assert eg <= 1e-6 and ej <= 1e-6 and eh <= 1e-6
    assert miss <= 1e-7
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', **kw)), bits(gT))          # (twice: the same bits)
    assert np.array_equal(bits(prob.JvecBorn(None, v, **kw)), bits(Jv))
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose', **FULL)), bits(gT))        # (u = None: the same launches)
    assert np.array_equal(bits(prob.JvecBorn(None, v, **FULL)), bits(Jv))
    assert rel(prob.Hvec(None, p, **FULL), Hp) <= 1e-12
    q = np.random.default_rng(37).standard_normal(prob.nrow)
    a, b = float(q @ Hp), float(p @ prob.Hvec(None, q, **kw))
    assert abs(a - b) <= 1e-7 * max(abs(a), abs(b)) and float(p @ Hp) > 0
    if density:
        kr = dict(u=F, parameter='rho')
        assert np.array_equal(bits(prob.JvecBorn(None, v, **kr, **FULL)), bits(prob.JvecBorn(None, v, linearisation='operator', **kr)))
    else:
        with pytest.raises(NotImplementedError):
            prob.JvecBorn(None, v, u=F, linearisation='operator')
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=F, **FULL)
    F.release()
    del prob.factors


@pytest.mark.parametrize('mode,density', ROUTES, ids=ROUTE_IDS)
def test_complex64_store_against_the_host_route_on_the_unpacked_fields(helm_lib, monkeypatch, host_ref, mode, density):
    "the format bound of test_gpu_frechet.py's complex64 test: the device on the packed store against the host route on the same, unpacked fields"
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[(mode, density)]
    v, r, probh = h['v'], h['r'], h['prob']
    prob64, sv64 = xc.pair(mode, E2E[mode], density=density, device=True, rtol=1e-11, fieldsDtype='complex64')
    F64 = prob64.fieldsDevice()
    assert F64.dtype == 'complex64'
    kw = dict(u=F64, **FULL)
    d64, g64 = prob64.JvecBorn(None, v, **kw), prob64.Jtvec(None, r, adjoint='transpose', **kw)
    unpacked = list(F64)
    dh = probh.JvecBorn(None, v, u=unpacked, **FULL)
    gh = probh.Jtvec(None, r, u=unpacked, adjoint='transpose', **FULL)
    print('%s %s complex64: JvecBorn against the host route on the unpacked fields %.2e, Jtvec %.2e' % (mode, density, rel(d64, dh), rel(g64, gh)))
    assert rel(d64, dh) <= 1e-6 and rel(g64, gh) <= 1e-6
    assert rel(d64, h['Jv']) > 0                                       # (the packed store was read)
    lhs = inner(d64, r)
    assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    F64.release()
    del prob64.factors


# ---- 3. Taylor through the device routes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
def test_taylor_remainder_of_the_device_dpred_falls_at_second_order(helm_lib, monkeypatch, density):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', False, density=density, device=True, rtol=1e-11)
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
    v = xc.perturbation()
    F = prob.fieldsDevice(c0)
    Jv = prob.JvecBorn(None, v, u=F, **FULL)
    F.release()
    r = xc.taylor_remainders(prob, sv, Jv, c0, v)
    print('device %s: remainders %s factors %s' % ('rho' if density else 'gardner', r, fc.factors(r)))
    assert all(f >= 3.5 for f in fc.factors(r))
    del prob.factors


# ---- 4. 'scaler', 'operator' and parameter='rho' are what they were ---------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', sorted(xc.RECORDED_MODES))
def test_the_other_linearisations_give_the_recorded_bits(helm_lib, monkeypatch, mode):
    "tests/golden/g13_operator_device.npz was written by tools/record_operator_device.py on the commit before linearisation='full' came"
    monkeypatch.setenv('HELM_DEVICES', '0')
    gold = np.load(xc.RECORDING)
    now = xc.recorded_products(mode)
    assert sorted('%s/%s' % (mode, k) for k in now) == sorted(k for k in gold.files if k.startswith(mode + '/'))
    for key, val in now.items():
        want = gold['%s/%s' % (mode, key)]
        assert val.dtype == want.dtype and val.shape == want.shape, key
        assert np.array_equal(bits(val), bits(want)), (key, rel(val, want))
