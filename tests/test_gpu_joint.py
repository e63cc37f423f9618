"""GPU: the stacked (c, rho) routes, parameter='joint', on the device -- k_mixed_adjoint and k_velocity_adjoint_b through their C entry points against the 80-bit
evaluations of tests/joint_cases.py under its componentwise bounds (both CONJ, both STRETCH, 3 x 3 included, zeros and both signs in p and B, guard cells, NaN
boundary rows, two runs the same bits), the device routes against the host routes fed the downloaded fields (fixed and moving arrays, both stores, 'full' and
'operator', one and two workers, u = F and u = None), the halves against the single-parameter device calls, and the central differences of the device gradient."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import joint_cases as jc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc = ac.rel, ac.randc
GUARD, FILL = 517, complex(7.0, -3.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. the two kernels ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_mixed_kernels_against_the_80_bit_evaluation(helm_lib, name):
    """G += w (conj-or-not M_b[p])^T P (k_mixed_adjoint) and G += w (conj-or-not M_c[B])^T P (k_velocity_adjoint_b) on assembled handles (3 x 3 -- every interior row
    touches a boundary --, 4 x 4, 5 x 63 with ky, 33 x 125: free-surface flags on and off, dx != dz, a damped frequency) per component within C_MIXED = 103 and
    C_VADJOINT_B = 95 times 2^-53 of the magnitudes of joint_cases, with and without the stretch part; p and B hold zeros and both signs; guard cells stay, G starts
    non-zero, the boundary rows of P are NaN, two runs give the same bits."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = dc.operator_config(name)
    op = za.MiniZephyr(dict(sc, device=0))
    p, B, Pl, G0 = jc.mixed_inputs(sc)
    N = p.size
    assert p.min() < 0 < p.max() and B.min() < 0 < B.max() and (N <= 9 or (np.any(p == 0) and np.any(B == 0)))
    dev = torch.device('cuda', 0)
    edge = ~np.asarray(dc.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    Pnan = Pl.copy()
    Pnan[:, edge] = complex(np.nan, np.nan)
    dp, dB, dP = torch.from_numpy(p).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(Pnan).to(dev)
    w = -0.7 + 0.4j
    kernels = {'k_mixed_adjoint': (helm_lib.helm_mixed_adjoint_device, dp, lambda *a: jc.mixed_b_reference(op, G0, Pl, p, *a), jc.C_MIXED),
               'k_velocity_adjoint_b': (helm_lib.helm_velocity_adjoint_b_device, dB, lambda *a: jc.mixed_c_reference(op, G0, Pl, B, *a), jc.C_VADJOINT_B)}
    worst, kept = {}, {}
    for kname, (f, dv, reference, count) in sorted(kernels.items()):
        for conj in (0, 1):
            for stretch in (0, 1):
                runs = []
                for _ in range(2):
                    buf = torch.full((2 * GUARD + N,), FILL, dtype=torch.complex128, device=dev)
                    buf[GUARD:GUARD + N] = torch.from_numpy(G0).to(dev)
                    torch.cuda.synchronize(dev)
                    d_g = P(buf.data_ptr() + 16 * GUARD)
                    _lib.check(f(op.handle, P(dP.data_ptr()), P(dv.data_ptr()), w.real, w.imag, conj, stretch, d_g), op.handle)
                    h = buf.cpu().numpy()
                    assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + N:] == FILL)
                    runs.append(h[GUARD:GUARD + N].copy())
                assert np.array_equal(bits(runs[0]), bits(runs[1]))
                assert np.all(np.isfinite(runs[0].view(np.float64)))                 # (the NaN boundary rows of P were not read)
                assert np.any(runs[0] != G0)
                ref, mag = reference(w, bool(conj), bool(stretch))
                worst['%s conj=%d stretch=%d' % (kname, conj, stretch)] = jc.worst_ratio(runs[0], ref, count * jc.U64 * mag)
                kept[(kname, conj, stretch)] = runs[0]
        # bad arguments are refused before anything is launched
        assert f(op.handle, P(dP.data_ptr()), P(dv.data_ptr()), 1.0, 0.0, 0, 1, P(dP.data_ptr() + 16)) == -1            # (G inside P)
        assert f(op.handle, P(dP.data_ptr() + 8), P(dv.data_ptr()), 1.0, 0.0, 0, 1, d_g) == -1
        assert f(op.handle, P(dP.data_ptr()), P(dv.data_ptr() + 4), 1.0, 0.0, 0, 1, d_g) == -1
        assert f(op.handle, P(dP.data_ptr()), P(dv.data_ptr()), 1.0, 0.0, 0, 1, P(d_g.value + 8)) == -1
        assert f(op.handle, None, P(dv.data_ptr()), 1.0, 0.0, 0, 1, d_g) == -1
        assert f(op.handle, P(dP.data_ptr()), None, 1.0, 0.0, 0, 1, d_g) == -1
        assert f(op.handle, P(dP.data_ptr()), P(dv.data_ptr()), 1.0, 0.0, 0, 1, None) == -1
        assert f(None, P(dP.data_ptr()), P(dv.data_ptr()), 1.0, 0.0, 0, 1, d_g) == -1
    print('%s: worst err / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    # through the method wrappers: the same bits
    for kname, call, dv in (('k_mixed_adjoint', op.mixedAdjointDevice, dp), ('k_velocity_adjoint_b', op.velocityAdjointBuoyancyDevice, dB)):
        buf = torch.from_numpy(G0).to(dev)
        torch.cuda.synchronize(dev)
        call(dP.data_ptr(), dv.data_ptr(), w, buf.data_ptr(), conj=True, stretch=True)
        assert np.array_equal(bits(buf.cpu().numpy()), bits(kept[(kname, 1, 1)]))
    # B = 1 / rho is k_velocity_adjoint: the same body at the buoyancy of the operator
    rho = np.asarray(sc['rho'], dtype=np.float64).ravel()
    a, b = torch.from_numpy(G0).to(dev), torch.from_numpy(G0).to(dev)
    dR = torch.from_numpy(1.0 / rho).to(dev)
    torch.cuda.synchronize(dev)
    op.velocityAdjointBuoyancyDevice(dP.data_ptr(), dR.data_ptr(), w, a.data_ptr(), conj=True, stretch=True)
    op.velocityAdjointDevice(dP.data_ptr(), w, b.data_ptr(), conj=True)
    assert rel(a.cpu().numpy(), b.cpu().numpy()) <= 1e-14
    del op.factors


def test_unassembled_small_eurus_and_3d_handles_are_refused(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    fs = (ctypes.c_int * 4)(0, 0, 0, 0)
    both = (helm_lib.helm_mixed_adjoint_device, helm_lib.helm_velocity_adjoint_b_device)
    a, b = torch.zeros(9 * 108, dtype=torch.complex128, device='cuda'), torch.zeros(108, dtype=torch.complex128, device='cuda')
    d = torch.zeros(108, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    raw = helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 12, 9, 10., 10., 2, fs)
    assert raw, _lib.last_error(None)
    for f in both:
        assert f(raw, P(a.data_ptr()), P(d.data_ptr()), 1.0, 0.0, 0, 1, P(b.data_ptr())) == -3          # (HELM_ERR_STATE: never assembled)
    helm_lib.helm_destroy(raw)
    # nz < 3 has no interior row: the entry points refuse such a grid, and the library makes no handle of one to begin with
    assert not helm_lib.helm_create(0, _lib.HELM_MINIZEPHYR, 2, 54, 10., 10., 1, fs)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, fs)
    assert eu, _lib.last_error(None)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for handle in (eu, h3.handle):
        N = int(helm_lib.helm_num_points(handle))
        g, c = torch.zeros(N, dtype=torch.complex128, device='cuda'), torch.zeros(9 * N, dtype=torch.complex128, device='cuda')
        dd = torch.zeros(N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        for f in both:
            assert f(handle, P(c.data_ptr()), P(dd.data_ptr()), 1.0, 0.0, 0, 1, P(g.data_ptr())) == -4
    helm_lib.helm_destroy(eu)
    del h3.factors


# ---- 2. the device routes against the host routes ----------------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm
ROUTES = [('fixed', 'full', 'complex128'), ('relative', 'full', 'complex64'), ('fixed', 'operator', 'complex64'), ('relative', 'operator', 'complex128')]


def _inputs(sv):
    vc, vr = jc.directions()
    return vc, vr, jc.stack(vc, vr), randc(np.random.default_rng(31), sv.nD)


@pytest.mark.parametrize('mode,lin,fmt', ROUTES, ids=['-'.join(r) for r in ROUTES])
def test_device_routes_against_the_host_routes_on_the_downloaded_fields(helm_lib, monkeypatch, mode, lin, fmt):
    """Jtvec, JvecBorn, Hvec() and Hvec(resid=r) with parameter='joint' and u = F within 1e-6 of the numpy routes fed the downloaded fields -- the tolerance of
    test_gpu_newton.py: up to three solves at rtol 1e-11 on either side -- for a random complex residual and perturbations non-zero in every cell; the halves
    against the single-parameter device calls to the same 1e-6; the same bits from a second call and (complex128 store) from u = None."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = jc.pair(mode, E2E[mode], device=True, rtol=1e-11, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    N = prob.nrow
    vc, vr, v, r = _inputs(sv)
    one = dict(linearisation=lin)
    kw = dict(one, parameter='joint')
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    host = list(F)
    calls = {'Jtvec': lambda u: prob.Jtvec(None, r, u=u, adjoint='transpose', **kw), 'JvecBorn': lambda u: prob.JvecBorn(None, v, u=u, **kw),
             'Hvec': lambda u: prob.Hvec(None, v, u=u, **kw), 'Newton': lambda u: prob.Hvec(None, v, u=u, resid=r, **kw)}
    got, err = {}, {}
    for name, call in calls.items():
        got[name] = call(F)
        err[name] = rel(got[name], call(host))
        assert np.array_equal(bits(call(F)), bits(got[name])), name
        if fmt == 'complex128':
            assert np.array_equal(bits(call(None)), bits(got[name])), name
    for name in ('Jtvec', 'Hvec', 'Newton'):
        assert got[name].shape == (2 * N,) and got[name].dtype == np.float64
    z = np.zeros(N)
    halves = {
        'Jtvec c': rel(got['Jtvec'][:N], prob.Jtvec(None, r, u=F, adjoint='transpose', parameter='c', **one)),
        'Jtvec rho': rel(got['Jtvec'][N:], prob.Jtvec(None, r, u=F, adjoint='transpose', parameter='rho', **one)),
        'JvecBorn': rel(got['JvecBorn'], prob.JvecBorn(None, vc, u=F, parameter='c', **one) + prob.JvecBorn(None, vr, u=F, parameter='rho', **one)),
        'Newton c': rel(prob.Hvec(None, jc.stack(vc, z), u=F, resid=r, **kw)[:N], prob.Hvec(None, vc, u=F, resid=r, parameter='c', **one)),
        'Newton rho': rel(prob.Hvec(None, jc.stack(z, vr), u=F, resid=r, **kw)[N:], prob.Hvec(None, vr, u=F, resid=r, parameter='rho', **one)),
        'resid = 0': rel(prob.Hvec(None, v, u=F, resid=np.zeros(sv.nD), **kw), got['Hvec'])}
    print('%s %s %s: device against host %s; against the single-parameter device calls %s; ||Hv - JtJv|| / ||Hv|| = %.2f' % (
        mode, lin, fmt, {k: '%.1e' % e for k, e in err.items()}, {k: '%.1e' % e for k, e in halves.items()}, fc.norm(got['Newton'] - got['Hvec']) / fc.norm(got['Newton'])))
    assert all(e <= 1e-6 for e in err.values()), err
    assert all(e <= 1e-6 for e in halves.values()), halves
    assert fc.norm(got['Newton'] - got['Hvec']) >= 0.1 * fc.norm(got['Newton'])
    F.release()
    del prob.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: the stacked partials are added on the host"
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    _, _, v, r = _inputs(sv)
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    for lin in ('full', 'operator'):
        kw = dict(linearisation=lin, parameter='joint')
        host = prob.Hvec(None, v, u=[F[0]], resid=r, **kw)
        for H in (prob.Hvec(None, v, u=F, resid=r, **kw), prob.Hvec(None, v, resid=r, **kw)):
            assert rel(H, host) <= 1e-6
        assert rel(prob.Jtvec(None, r, u=F, adjoint='transpose', **kw), prob.Jtvec(None, r, u=[F[0]], adjoint='transpose', **kw)) <= 1e-6
        assert rel(prob.Hvec(None, v, u=F, **kw), prob.Hvec(None, v, u=[F[0]], **kw)) <= 1e-6
    F.release()
    del prob.factors


# ---- 3. central differences of the device gradient ------------------------------------------------------------------------------------------------------
def test_central_differences_of_the_device_joint_gradient_converge_to_the_device_newton_product(helm_lib, monkeypatch):
    "test 3 of test_joint_host.py through the device routes: dpred, the joint Jtvec and the joint Hvec(resid=) all with the fields in HBM, 'full', both halves of v"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = jc.pair('fixed', False, device=True, rtol=1e-11)
    N = prob.nrow
    dobs = jc.observed(prob, sv)
    vc, vr = jc.directions()
    v = jc.stack(vc, vr)
    kw = dict(linearisation='full', parameter='joint')
    F = prob.fieldsDevice()
    r = sv.dpred(None, u=F) - dobs
    Hv, Hgn = prob.Hvec(None, v, u=F, resid=r, **kw), prob.Hvec(None, v, u=F, **kw)
    F.release()
    g = jc.gradient_of(prob, sv, dobs, linearisation='full')
    rn = jc.central_remainders(g, v, Hv, N)
    jc.restore(prob)
    print('device joint: remainders %s factors %s / %s; ||Hv - JtJv|| / ||Hv|| = %.3f' % (rn, fc.factors([x[0] for x in rn]), fc.factors([x[1] for x in rn]),
                                                                                          fc.norm(Hv - Hgn) / fc.norm(Hv)))
    for half in (0, 1):
        assert all(f >= jc.SECOND for f in fc.factors([x[half] for x in rn]))
    del prob.factors
