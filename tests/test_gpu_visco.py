"""GPU: the exact velocity and Q derivatives of a visco problem on the device -- k_visco_perturbation, k_velocity_planes_z and k_visco_chain_adjoint through their C
entry points against the 80-bit evaluations of tests/visco_cases.py under its componentwise bounds (Q rough with infinite cells, lam non-zero and zero, every NULL
combination, conj 0 and 1, guard cells, two runs the same bits), the refusals of the entry points, the device routes of JvecBorn / Jtvec / Hvec against the host
route on the oracle doubles (both stores, fixed and moving arrays, u = F and u = None, two workers), and the Taylor test of dpred through the device routes."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import visco_cases as vc
from zephyr_amd import frechet as fr

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc, inner = ac.rel, ac.randc, ac.inner
T = dict(adjoint='transpose')
LAMS = (0.091, 0.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _visco_operator(name, lam):
    "an assembled handle of dc.OPERATOR_CASES holding the complex velocity of (c, Q, lam), with the real model beside it"
    import zephyr_amd as za
    sc = dc.operator_config(name)
    c, Q = vc.kernel_model(sc)
    ct = vc.complex_velocity(c, Q, lam)
    op = za.MiniZephyr(dict(sc, c=ct.reshape((sc['nz'], sc['nx'])), device=0))
    op.handle
    return sc, op, c, Q, ct


# ---- 1. the three kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam', LAMS, ids=['dispersion', 'flat'])
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_visco_kernels_against_the_80_bit_evaluation(helm_lib, name, lam):
    """dc~ = gamma vc + chi vQ, dC = V[dc~] and (Gc, GQ) += (gamma`, chi`) T on assembled handles (3 x 3, 4 x 4, 5 x 63 -- N = 315 crosses one 256-thread block --
    and 33 x 125) per component within C_PERTURB, C_VPLANES_Z and C_CHAINADJ times 2^-53 of the magnitudes of visco_cases; guard cells stay, G starts non-zero,
    two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    sc, op, c, Q, ct = _visco_operator(name, lam)
    N = c.size
    rng = np.random.default_rng(13)
    a, b = rng.uniform(-50., 50., N), rng.uniform(-2., 2., N)
    Tc, G0 = randc(rng, N), randc(rng, (2, N))
    dev = torch.device('cuda', 0)
    guard, fill = 517, complex(7.0, -3.0)
    dQ, dA, dB, dT = (torch.from_numpy(x).to(dev) for x in (Q, a, b, Tc))
    worst = {}
    # k_visco_perturbation: both halves, and each alone
    last = None
    for label, pa, pb, ha, hb in (('both', P(dA.data_ptr()), P(dB.data_ptr()), a, b), ('c alone', P(dA.data_ptr()), None, a, None), ('Q alone', None, P(dB.data_ptr()), None, b)):
        runs = []
        for _ in range(2):
            out = torch.full((2 * guard + N,), fill, dtype=torch.complex128, device=dev)
            torch.cuda.synchronize(dev)
            _lib.check(helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr()), lam, pa, pb, P(out.data_ptr() + 16 * guard)), op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + N:] == fill)
            runs.append(h[guard:guard + N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = vc.perturbation_reference(ct, Q, lam, ha, hb)
        worst['perturbation ' + label] = vc.worst_ratio(runs[0], ref, vc.C_PERTURB * vc.U64 * mag)
        if hb is not None and lam != 0.0:
            assert vc.worst_ratio(vc.perturbation_reference(ct, Q, lam, ha, hb, dispersion=False)[0], ref, vc.C_PERTURB * vc.U64 * mag) > 1e6      # (on the CPU: a wrong chi)
        if ha is None:
            assert np.all(runs[0][np.isinf(Q)] == 0)                     # (Q = inf: chi = 0, no NaN from an infinity)
        if label == 'both':
            last = runs[0]
    # k_velocity_planes_z on the perturbation the first kernel made
    dZ = torch.from_numpy(last).to(dev)
    runs = []
    for _ in range(2):
        out = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
        torch.cuda.synchronize(dev)
        d_c = P(out.data_ptr() + 16 * guard)
        _lib.check(helm_lib.helm_velocity_planes_z_device(op.handle, P(dZ.data_ptr()), d_c), op.handle)
        h = out.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
        runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    edge = ~np.asarray(fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    assert np.all(runs[0][:, edge] == 0)
    ref, mag = vc.planes_z_reference(op, last)
    worst['planes'] = vc.worst_ratio(runs[0], ref, vc.C_VPLANES_Z * vc.U64 * mag)
    # k_visco_chain_adjoint: both outputs, and each alone
    for conj in (0, 1):
        for label, wc, wq in (('both', True, True), ('c alone', True, False), ('Q alone', False, True)):
            runs = []
            for _ in range(2):
                buf = torch.full((2, 2 * guard + N), fill, dtype=torch.complex128, device=dev)
                buf[:, guard:guard + N] = torch.from_numpy(G0).to(dev)
                torch.cuda.synchronize(dev)
                pc = P(buf[0].data_ptr() + 16 * guard) if wc else None
                pq = P(buf[1].data_ptr() + 16 * guard) if wq else None
                _lib.check(helm_lib.helm_visco_chain_adjoint_device(op.handle, P(dQ.data_ptr()), lam, P(dT.data_ptr()), conj, pc, pq), op.handle)
                h = buf.cpu().numpy()
                assert np.all(h[:, :guard] == fill) and np.all(h[:, guard + N:] == fill)
                runs.append(h[:, guard:guard + N].copy())
            assert np.array_equal(bits(runs[0]), bits(runs[1]))
            refs = vc.chain_adjoint_reference(ct, Q, lam, Tc, G0, bool(conj))
            for row, want, (ref, mag) in ((0, wc, refs[0]), (1, wq, refs[1])):
                if want:
                    worst['adjoint %s conj=%d %s' % (label, conj, 'cQ'[row])] = vc.worst_ratio(runs[0][row], ref, vc.C_CHAINADJ * vc.U64 * mag)
                else:
                    assert np.array_equal(bits(runs[0][row]), bits(G0[row]))         # (a NULL output is left alone)
    print('%s lam=%g: worst err / bound %.3f (%s)' % (name, lam, max(worst.values()), ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    # bad arguments are refused before anything is launched
    d_z, d_t = P(dZ.data_ptr()), P(dT.data_ptr())
    assert helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr()), lam, None, None, d_z) == -1
    assert helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr() + 4), lam, P(dA.data_ptr()), None, d_z) == -1
    assert helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr()), lam, P(dA.data_ptr()), None, P(dZ.data_ptr() + 8)) == -1
    assert helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr()), lam, P(dA.data_ptr()), None, P(dA.data_ptr())) == -1
    assert helm_lib.helm_visco_perturbation_device(op.handle, P(dQ.data_ptr()), float('nan'), P(dA.data_ptr()), None, d_z) == -1
    assert helm_lib.helm_velocity_planes_z_device(op.handle, d_z, d_z) == -1
    assert helm_lib.helm_velocity_planes_z_device(op.handle, P(dZ.data_ptr() + 8), d_c) == -1
    assert helm_lib.helm_velocity_planes_z_device(op.handle, None, d_c) == -1
    assert helm_lib.helm_visco_chain_adjoint_device(op.handle, P(dQ.data_ptr()), lam, d_t, 0, None, None) == -1
    assert helm_lib.helm_visco_chain_adjoint_device(op.handle, P(dQ.data_ptr()), lam, d_t, 0, d_t, None) == -1
    assert helm_lib.helm_visco_chain_adjoint_device(op.handle, P(dQ.data_ptr()), lam, d_t, 0, d_z, d_z) == -1
    assert helm_lib.helm_visco_chain_adjoint_device(op.handle, P(dQ.data_ptr()), lam, d_t, 0, P(dZ.data_ptr() + 8), None) == -1
    del op.factors


def test_unassembled_eurus_and_3d_handles_are_refused(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert raw, _lib.last_error(None)
    z, g, c9 = (torch.zeros(n, dtype=torch.complex128, device='cuda') for n in (108, 108, 9 * 108))
    q = torch.ones(108, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert helm_lib.helm_visco_perturbation_device(raw, P(q.data_ptr()), 0.1, P(q.data_ptr()), None, P(z.data_ptr())) == -3          # (no assembled operator: HELM_ERR_STATE)
    assert helm_lib.helm_velocity_planes_z_device(raw, P(z.data_ptr()), P(c9.data_ptr())) == -3
    assert helm_lib.helm_visco_chain_adjoint_device(raw, P(q.data_ptr()), 0.1, P(z.data_ptr()), 1, P(g.data_ptr()), None) == -3
    helm_lib.helm_destroy(raw)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for handle in (eu, h3.handle):
        N = int(helm_lib.helm_num_points(handle))
        z, g, c9 = (torch.zeros(n, dtype=torch.complex128, device='cuda') for n in (N, N, 9 * N))
        q = torch.ones(N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        assert helm_lib.helm_visco_perturbation_device(handle, P(q.data_ptr()), 0.1, P(q.data_ptr()), None, P(z.data_ptr())) == -4
        assert helm_lib.helm_velocity_planes_z_device(handle, P(z.data_ptr()), P(c9.data_ptr())) == -4
        assert helm_lib.helm_visco_chain_adjoint_device(handle, P(q.data_ptr()), 0.1, P(z.data_ptr()), 1, P(g.data_ptr()), None) == -4
    helm_lib.helm_destroy(eu)
    del h3.factors


# ---- 2. the device routes against the host route -----------------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm
ALL = vc.PARAMETERS + ('rho',)


def _vector(parameter, a, b, d):
    return d if parameter == 'rho' else vc.stacked(parameter, a, b)


@pytest.fixture(scope='module')
def host_ref():
    'per mode, from the oracle doubles on the host route, made once: perturbations non-zero everywhere, a residual and the products per parameter and linearisation'
    out = {}
    for mode in E2E:
        probh, svh = vc.pair(vc.strong_config(mode, E2E[mode]))
        rng = np.random.default_rng(31)
        a, b = vc.perturbations()
        d, r = dc.perturbation(), randc(rng, svh.nD)
        uF = probh.fields()
        res = {}
        for par in ALL:
            for lin in ('full', 'operator'):
                kw = dict(u=uF, linearisation=lin, parameter=par)
                res[(par, lin)] = (probh.JvecBorn(None, _vector(par, a, b, d), **kw), probh.Jtvec(None, r, **T, **kw))
        out[mode] = dict(prob=probh, sv=svh, a=a, b=b, d=d, r=r, res=res)
    return out


@pytest.mark.parametrize('mode', sorted(E2E))
def test_device_routes_against_the_host_route_with_the_store_and_without(helm_lib, monkeypatch, host_ref, mode):
    """complex128 store, rtol 1e-11: 1e-6 against the host route and the identity at 1e-7, the tolerances of test_gpu_full.py, for 'c', 'Q', 'cQ' and 'rho' with
    'full' and 'operator'; u = None gives the same bits as u = F; two consecutive calls give the same bits; Hvec is the composition."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    a, b, d, r = h['a'], h['b'], h['d'], h['r']
    prob, sv = vc.pair(vc.strong_config(mode, E2E[mode], device=True, rtol=1e-11))
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    for par in ALL:
        n = prob.nrow * (2 if par == 'cQ' else 1)
        v = _vector(par, a, b, d)
        for lin in ('full', 'operator'):
            kw = dict(u=F, linearisation=lin, parameter=par)
            Jv, gT = prob.JvecBorn(None, v, **kw), prob.Jtvec(None, r, **T, **kw)
            assert gT.shape == (n,) and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128
            ej, eg = rel(Jv, h['res'][(par, lin)][0]), rel(gT, h['res'][(par, lin)][1])
            lhs = inner(Jv, r)
            miss = abs(lhs - inner(v, gT)) / abs(lhs)
            print('%s %s %s: JvecBorn against the host route %.2e, Jtvec %.2e; identity misses by %.2e' % (mode, par, lin, ej, eg, miss))
            assert ej <= 1e-6 and eg <= 1e-6 and miss <= 1e-7
            assert np.array_equal(bits(prob.Jtvec(None, r, **T, **kw)), bits(gT)) and np.array_equal(bits(prob.JvecBorn(None, v, **kw)), bits(Jv))      # (twice)
            if lin == 'full':
                none = dict(linearisation=lin, parameter=par)
                assert np.array_equal(bits(prob.Jtvec(None, r, **T, **none)), bits(gT)) and np.array_equal(bits(prob.JvecBorn(None, v, **none)), bits(Jv))      # (u = None)
    kw = dict(u=F, linearisation='full', parameter='cQ')
    p = np.random.default_rng(37).standard_normal(2 * prob.nrow)
    Hp = prob.Hvec(None, p, **kw)
    assert np.array_equal(bits(Hp), bits(prob.Jtvec(None, prob.JvecBorn(None, p, **kw), **T, **kw))) and float(p @ Hp) > 0
    g = prob.Jtvec(None, r, **T, **kw)
    halves = np.concatenate([prob.Jtvec(None, r, **T, **dict(kw, parameter='c')), prob.Jtvec(None, r, **T, **dict(kw, parameter='Q'))])
    assert rel(g, halves) <= 1e-12
    F.release()
    del prob.factors


@pytest.mark.parametrize('mode', sorted(E2E))
def test_complex64_store_against_the_host_route_on_the_unpacked_fields(helm_lib, monkeypatch, host_ref, mode):
    "the format bound of test_gpu_full.py's complex64 test: the device on the packed store against the host route on the same, unpacked fields"
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    a, b, r, probh = h['a'], h['b'], h['r'], h['prob']
    v = vc.stacked('cQ', a, b)
    prob64, sv64 = vc.pair(vc.strong_config(mode, E2E[mode], device=True, rtol=1e-11, fieldsDtype='complex64'))
    F64 = prob64.fieldsDevice()
    assert F64.dtype == 'complex64'
    unpacked = list(F64)
    for lin in ('full', 'operator'):
        kw = dict(linearisation=lin, parameter='cQ')
        d64, g64 = prob64.JvecBorn(None, v, u=F64, **kw), prob64.Jtvec(None, r, u=F64, **T, **kw)
        dh, gh = probh.JvecBorn(None, v, u=unpacked, **kw), probh.Jtvec(None, r, u=unpacked, **T, **kw)
        print('%s %s complex64: JvecBorn against the host route on the unpacked fields %.2e, Jtvec %.2e' % (mode, lin, rel(d64, dh), rel(g64, gh)))
        assert rel(d64, dh) <= 1e-6 and rel(g64, gh) <= 1e-6
        assert rel(d64, h['res'][('cQ', lin)][0]) > 0                                       # (the packed store was read)
        lhs = inner(d64, r)
        assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    F64.release()
    del prob64.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: the stacked partials are added on the host"
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = vc.strong_config('fixed', True, device=True, rtol=1e-11)
    sc.update(freqs=[7.], sterms=np.array([0.8 - 0.3j]))
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = vc.pair(sc)
    assert len(prob.system.devices) == 2
    a, b = vc.perturbations()
    v, r = vc.stacked('cQ', a, b), randc(np.random.default_rng(5), sv.nD)
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    for lin in ('full', 'operator'):
        kw = dict(linearisation=lin, parameter='cQ')
        assert rel(prob.Jtvec(None, r, u=F, **T, **kw), prob.Jtvec(None, r, u=[F[0]], **T, **kw)) <= 1e-6
        assert rel(prob.JvecBorn(None, v, u=F, **kw), prob.JvecBorn(None, v, u=[F[0]], **kw)) <= 1e-6
    F.release()
    del prob.factors


# ---- 3. Taylor through the device routes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parameter', vc.PARAMETERS)
def test_taylor_remainder_of_the_device_dpred_falls_at_second_order(helm_lib, monkeypatch, parameter):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = vc.pair(vc.strong_config(device=True, rtol=1e-11))
    a, b = vc.perturbations()
    F = prob.fieldsDevice()
    Jv = prob.JvecBorn(None, vc.stacked(parameter, a, b), u=F, linearisation='full', parameter=parameter)
    F.release()
    r = vc.taylor_remainders(prob, sv, Jv, parameter, a, b)
    print('device %s: remainders %s factors %s' % (parameter, r, fc.factors(r)))
    assert len(r) == 6 and all(f >= 3.5 for f in fc.factors(r))
    del prob.factors
