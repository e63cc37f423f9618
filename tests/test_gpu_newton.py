"""GPU: the full Newton Hessian-vector product, Hvec(resid=), on the device -- k_velocity_curvature and k_stencil_sources_t through their C entry points against the
80-bit evaluations of tests/newton_cases.py under its componentwise bounds (both CONJ, both STRETCH, both store formats, every shape at which the walk takes
another path, 3 x 3 included, guard cells, two runs the same bits), the device route against the host route fed the downloaded fields (fixed and moving arrays,
one and two workers, u = F and u = None), the central differences of the device gradient, and the routes that must stay as they were against their recording."""
import ctypes

import numpy as np
import pytest

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from tests import newton_cases as nc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc = ac.rel, ac.randc
GUARD, FILL = 517, complex(7.0, -3.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class RawHandle(object):
    'a library handle of a grid, created and never assembled: the transposed stencil reads the grid and the stream of a handle, not its operator'

    def __init__(self, lib, variant, nz, nx):
        from zephyr_amd import _lib
        self.lib, self.device = lib, 0
        self.handle = lib.helm_create(0, variant, nz, nx, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
        assert self.handle, _lib.last_error(None)

    def close(self):
        self.lib.helm_destroy(self.handle)


# ---- 1. k_velocity_curvature ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_curvature_kernel_against_the_80_bit_evaluation(helm_lib, name):
    """G += w p (.) (conj-or-not d2A)^T P on assembled handles (3 x 3 -- every interior row touches a boundary --, 4 x 4, 5 x 63, 33 x 125: free-surface flags on
    and off, dx != dz, ky, a damped frequency) per component within C_CURVATURE = 107 times 2^-53 of the magnitude of newton_cases, with and without the stretch
    part; guard cells stay, G starts non-zero, the boundary rows of P are NaN, two runs give the same bits."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = dc.operator_config(name)
    op = za.MiniZephyr(dict(sc, device=0))
    p, Pl, G0 = nc.curvature_inputs(sc)
    N = p.size
    dev = torch.device('cuda', 0)
    edge = ~np.asarray(dc.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    Pnan = Pl.copy()
    Pnan[:, edge] = complex(np.nan, np.nan)
    dp, dP = torch.from_numpy(p).to(dev), torch.from_numpy(Pnan).to(dev)
    w = -0.7 + 0.4j
    worst = {}
    for conj in (0, 1):
        for stretch in (0, 1):
            runs = []
            for _ in range(2):
                buf = torch.full((2 * GUARD + N,), FILL, dtype=torch.complex128, device=dev)
                buf[GUARD:GUARD + N] = torch.from_numpy(G0).to(dev)
                torch.cuda.synchronize(dev)
                d_g = P(buf.data_ptr() + 16 * GUARD)
                _lib.check(helm_lib.helm_velocity_curvature_device(op.handle, P(dP.data_ptr()), P(dp.data_ptr()), w.real, w.imag, conj, stretch, d_g), op.handle)
                h = buf.cpu().numpy()
                assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + N:] == FILL)
                runs.append(h[GUARD:GUARD + N].copy())
            assert np.array_equal(bits(runs[0]), bits(runs[1]))
            assert np.all(np.isfinite(runs[0].view(np.float64)))                 # (the NaN boundary rows of P were not read)
            assert np.any(runs[0] != G0)
            ref, mag = nc.curvature_reference(op, G0, Pl, p, w, bool(conj), bool(stretch))
            worst['conj=%d stretch=%d' % (conj, stretch)] = nc.worst_ratio(runs[0], ref, nc.C_CURVATURE * nc.U64 * mag)
    print('%s: k_velocity_curvature worst err / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    # through the method wrapper: the same bits
    buf = torch.from_numpy(G0).to(dev)
    torch.cuda.synchronize(dev)
    op.velocityCurvatureDevice(dP.data_ptr(), dp.data_ptr(), w, buf.data_ptr(), conj=True, stretch=True)
    assert np.array_equal(bits(buf.cpu().numpy()), bits(runs[0]))
    # bad arguments are refused before anything is launched
    f = helm_lib.helm_velocity_curvature_device
    assert f(op.handle, P(dP.data_ptr()), P(dp.data_ptr()), 1.0, 0.0, 0, 1, P(dP.data_ptr() + 16)) == -1
    assert f(op.handle, P(dP.data_ptr() + 8), P(dp.data_ptr()), 1.0, 0.0, 0, 1, d_g) == -1
    assert f(op.handle, P(dP.data_ptr()), P(dp.data_ptr() + 4), 1.0, 0.0, 0, 1, d_g) == -1
    assert f(op.handle, P(dP.data_ptr()), None, 1.0, 0.0, 0, 1, d_g) == -1
    assert f(op.handle, P(dP.data_ptr()), P(dp.data_ptr()), 1.0, 0.0, 0, 1, None) == -1
    del op.factors


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_mass_term_kernels_against_the_80_bit_evaluation(helm_lib, name):
    """k_mass_planes and the mass-only k_velocity_adjoint (linearisation='operator') on the four assembled handles: per component within C_MPLANES = 18 and
    full_cases.C_VADJOINT = 98 times 2^-53 of the magnitudes of newton_cases; boundary rows zero, guard cells stay, NaN boundary rows of P, two runs the same bits;
    the planes are not those of k_velocity_planes wherever the grid has a stretched cell."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = dc.operator_config(name)
    op = za.MiniZephyr(dict(sc, device=0))
    v, _, Pl, G0 = xc.operator_inputs(sc)
    N = v.size
    dev = torch.device('cuda', 0)
    edge = ~np.asarray(dc.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
    Pnan = Pl.copy()
    Pnan[:, edge] = complex(np.nan, np.nan)
    dV, dP = torch.from_numpy(v).to(dev), torch.from_numpy(Pnan).to(dev)
    worst, runs = {}, []
    for _ in range(2):
        out = torch.full((2 * GUARD + 9 * N,), FILL, dtype=torch.complex128, device=dev)
        torch.cuda.synchronize(dev)
        op.massPlanesDevice(dV.data_ptr(), out.data_ptr() + 16 * GUARD)
        h = out.cpu().numpy()
        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + 9 * N:] == FILL)
        runs.append(h[GUARD:GUARD + 9 * N].reshape((9, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.all(runs[0][:, edge] == 0)
    ref, mag = nc.mass_planes_reference(op, v)
    worst['planes'] = nc.worst_ratio(runs[0], ref, nc.C_MPLANES * nc.U64 * mag)
    full = xc.planes_reference(op, v)[0]
    assert nc.worst_ratio(runs[0], full, nc.C_MPLANES * nc.U64 * mag) > 1e6          # (every one of these grids has cells in the absorbing layers)
    w = -0.7 + 0.4j
    for conj in (False, True):
        runs = []
        for _ in range(2):
            buf = torch.full((2 * GUARD + N,), FILL, dtype=torch.complex128, device=dev)
            buf[GUARD:GUARD + N] = torch.from_numpy(G0).to(dev)
            torch.cuda.synchronize(dev)
            op.massAdjointDevice(dP.data_ptr(), w, buf.data_ptr() + 16 * GUARD, conj=conj)
            h = buf.cpu().numpy()
            assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + N:] == FILL)
            runs.append(h[GUARD:GUARD + N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.all(np.isfinite(runs[0].view(np.float64)))
        ref, mag = nc.mass_adjoint_reference(op, G0, Pl, w, conj)
        worst['adjoint conj=%d' % conj] = nc.worst_ratio(runs[0], ref, nc.C_VADJOINT * nc.U64 * mag)
    print('%s: mass term worst err / bound %s' % (name, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    assert helm_lib.helm_mass_planes_device(op.handle, P(dV.data_ptr() + 4), P(out.data_ptr())) == -1
    assert helm_lib.helm_mass_planes_device(op.handle, None, P(out.data_ptr())) == -1
    assert helm_lib.helm_mass_adjoint_device(op.handle, P(dP.data_ptr()), 1.0, 0.0, 0, P(dP.data_ptr() + 16)) == -1
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
    assert helm_lib.helm_velocity_curvature_device(raw, P(a.data_ptr()), P(d.data_ptr()), 1.0, 0.0, 0, 1, P(b.data_ptr())) == -3          # (HELM_ERR_STATE)
    assert helm_lib.helm_mass_planes_device(raw, P(d.data_ptr()), P(a.data_ptr())) == -3
    assert helm_lib.helm_mass_adjoint_device(raw, P(a.data_ptr()), 1.0, 0.0, 0, P(b.data_ptr())) == -3
    helm_lib.helm_destroy(raw)
    eu = helm_lib.helm_create(0, _lib.HELM_EURUS, 36, 40, 10., 10., 2, (ctypes.c_int * 4)(0, 0, 0, 0))
    assert eu, _lib.last_error(None)
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    for handle in (eu, h3.handle):
        N = int(helm_lib.helm_num_points(handle))
        g, u = torch.zeros(N, dtype=torch.complex128, device='cuda'), torch.zeros(N, dtype=torch.complex128, device='cuda')
        c = torch.zeros(9 * N, dtype=torch.complex128, device='cuda')
        d = torch.zeros(N, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        assert helm_lib.helm_velocity_curvature_device(handle, P(c.data_ptr()), P(d.data_ptr()), 1.0, 0.0, 0, 1, P(g.data_ptr())) == -4
        assert helm_lib.helm_stencil_sources_t_device(handle, P(u.data_ptr()), 1, N, P(c.data_ptr()), 1.0, 0.0, 0, 0, P(g.data_ptr()), N) == -4
        assert helm_lib.helm_mass_planes_device(handle, P(d.data_ptr()), P(c.data_ptr())) == -4
        assert helm_lib.helm_mass_adjoint_device(handle, P(c.data_ptr()), 1.0, 0.0, 0, P(g.data_ptr())) == -4
    helm_lib.helm_destroy(eu)
    del h3.factors


# ---- 2. k_stencil_sources_t --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('case', nc.KERNEL_CASES, ids=['%dx%dx%d' % c for c in nc.KERNEL_CASES])
def test_transposed_stencil_against_the_80_bit_evaluation(helm_lib, case, fmt):
    """R = coef (conj-or-not C)^T U per component within C_STENCIL_T = 21 times 2^-53 of the magnitude of newton_cases, plus 2^-24 of it for the complex64 store.
    The shapes of density_cases.KERNEL_CASES: 3 x 3, nx either side of the lane tiling (61 .. 64, 125), a second chunk of rows (33), nsrc 1, 4, 5, 33 (partial
    groups of the column block).  The planes are random on the boundary rows too: the kernel reads what it is given.  Leading dimensions > N; guard cells and the
    gaps between columns stay as they were; two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference
    nz, nx, nsrc = case
    op = RawHandle(helm_lib, _lib.HELM_MINIZEPHYR, nz, nx)
    dev = torch.device('cuda', op.device)
    N = nz * nx
    ldu, ldr = N + 38, N + 11
    U, _, C, _ = nc.kernel_inputs(nz, nx, nsrc, seed=100 * nz + nx + nsrc)
    coef = 0.3 - 1.1j
    fterm = 2.0 ** -24 if fmt == 'complex64' else 0.0
    dC = torch.from_numpy(C).to(dev)
    if fmt == 'complex64':
        Pk, e = pack_reference(np.ascontiguousarray(U.T))
        Ppad = np.zeros((nsrc, ldu), dtype=np.complex64)
        Ppad[:, :N] = Pk.T
        dU, dE = torch.from_numpy(Ppad).to(dev), torch.from_numpy(e).to(dev)
    else:
        Upad = np.zeros((nsrc, ldu), dtype=np.complex128)
        Upad[:, :N] = U
        dU, dE = torch.from_numpy(Upad).to(dev), None

    def call(conj, d_r, u=None, nsrc_=nsrc, ldu_=ldu, ldr_=ldr, acc=0):
        u = dU.data_ptr() if u is None else u
        if fmt == 'complex64':
            return helm_lib.helm_stencil_sources_t_c64_device(op.handle, P(u), P(dE.data_ptr()), nsrc_, ldu_, P(dC.data_ptr()), coef.real, coef.imag, conj, acc, d_r, ldr_)
        return helm_lib.helm_stencil_sources_t_device(op.handle, P(u), nsrc_, ldu_, P(dC.data_ptr()), coef.real, coef.imag, conj, acc, d_r, ldr_)
    worst = {}
    for conj in (0, 1):
        runs = []
        for _ in range(2):
            out = torch.full((2 * GUARD + nsrc * ldr,), FILL, dtype=torch.complex128, device=dev)
            torch.cuda.synchronize(dev)
            d_r = P(out.data_ptr() + 16 * GUARD)
            _lib.check(call(conj, d_r), op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + nsrc * ldr:] == FILL)
            body = h[GUARD:GUARD + nsrc * ldr].reshape((nsrc, ldr))
            assert np.all(body[:, N:] == FILL)
            runs.append(body[:, :N].copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = nc.stencil_t_reference(U, C, coef, nz, nx, bool(conj))
        worst['conj=%d' % conj] = nc.worst_ratio(runs[0], ref, (nc.C_STENCIL_T * nc.U64 + fterm) * mag)
        # accumulate: the conjugate is added to what R holds, the gaps between the columns left as they are
        R0 = np.full((nsrc, ldr), FILL, dtype=np.complex128)
        R0[:, :N] = randc(np.random.default_rng(7 + conj), (nsrc, N)) * float(np.median(np.asarray(mag, dtype=np.float64)))
        out = torch.from_numpy(R0.ravel().copy()).to(dev)
        torch.cuda.synchronize(dev)
        _lib.check(call(conj, P(out.data_ptr()), acc=1), op.handle)
        body = out.cpu().numpy().reshape((nsrc, ldr))
        assert np.all(body[:, N:] == FILL)
        aref, amag = nc.stencil_t_accumulated(R0[:, :N], ref, mag)
        worst['accumulate conj=%d' % conj] = nc.worst_ratio(body[:, :N], aref, (nc.C_STENCIL_T + 1) * nc.U64 * amag + fterm * mag)
    print('%dx%d nsrc=%d %s: k_stencil_sources_t worst err / bound %s' % (nz, nx, nsrc, fmt, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(w <= 1.0 for w in worst.values()), worst
    # bad arguments are refused before anything is launched
    assert call(0, d_r, ldu_=N - 1) == -1 and call(0, d_r, nsrc_=0) == -1 and call(0, d_r, ldr_=N - 1) == -1
    assert call(0, P(d_r.value + 8)) == -1 and call(0, P(dC.data_ptr() + 16), ldr_=N) == -1 and call(0, None) == -1
    assert call(0, d_r, u=dU.data_ptr() + 4) == -1
    op.close()


# ---- 3. the device route against the host route --------------------------------------------------------------------------------------------------------
E2E = {'fixed': False, 'relative': True}          # mode -> the HD class with a complex scaleTerm
ROUTES = [('fixed', 'full', 'c', 'complex128'), ('relative', 'full', 'c', 'complex128'), ('fixed', 'operator', 'rho', 'complex128'), ('relative', 'full', 'rho', 'complex64'),
          ('fixed', 'full', 'c', 'complex64'), ('fixed', 'operator', 'c', 'complex128'), ('relative', 'operator', 'c', 'complex64')]


def _inputs(prob, sv, par):
    rng = np.random.default_rng(31)
    p = dc.perturbation() if par == 'rho' else nc.everywhere()
    return p, randc(rng, sv.nD)


@pytest.mark.parametrize('mode,lin,par,fmt', ROUTES, ids=['-'.join(r) for r in ROUTES])
def test_device_route_against_the_host_route_on_the_downloaded_fields(helm_lib, monkeypatch, mode, lin, par, fmt):
    """Hvec(u=F, resid=r) within 1e-6 of the numpy route fed the downloaded fields -- the tolerance of the device-against-host tests of test_gpu_full.py: three
    solves at rtol 1e-11 on either side -- for a random complex residual and a perturbation non-zero everywhere.  The same bits from a second call and (complex128
    store) from u = None; resid = 0 is the Gauss-Newton product to the same 1e-6."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair(mode, E2E[mode], device=True, rtol=1e-11, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    p, r = _inputs(prob, sv, par)
    kw = dict(linearisation=lin, parameter=par)
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    Hp = prob.Hvec(None, p, u=F, resid=r, **kw)
    assert Hp.shape == (prob.nrow,) and Hp.dtype == np.float64
    host = prob.Hvec(None, p, u=list(F), resid=r, **kw)
    gn = prob.Hvec(None, p, u=F, **kw)
    e_host, e_zero = rel(Hp, host), rel(prob.Hvec(None, p, u=F, resid=np.zeros(sv.nD), **kw), gn)
    print('%s %s %s %s: device against host %.2e, resid = 0 against Gauss-Newton %.2e, ||Hp - JtJp|| / ||Hp|| = %.2f' % (mode, lin, par, fmt, e_host, e_zero,
                                                                                                                     fc.norm(Hp - gn) / fc.norm(Hp)))
    assert e_host <= 1e-6 and e_zero <= 1e-6
    assert fc.norm(Hp - gn) >= 0.1 * fc.norm(Hp)
    assert np.array_equal(bits(prob.Hvec(None, p, u=F, resid=r, **kw)), bits(Hp))
    if fmt == 'complex128':
        assert np.array_equal(bits(prob.Hvec(None, p, resid=r, **kw)), bits(Hp))
    q = np.random.default_rng(37).standard_normal(prob.nrow)
    a, b = float(q @ Hp), float(p @ prob.Hvec(None, q, u=F, resid=r, **kw))
    assert abs(a - b) <= 1e-7 * max(abs(a), abs(b))                     # (the symmetry bound of test_gpu_full.py on the device)
    F.release()
    del prob.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: the partials are added on the host"
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = fc.config('fixed', True, Disc=za.MiniZephyrHD, freqs=[fc.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    p, r = _inputs(prob, sv, 'c')
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    for kw in (dict(linearisation='full'), dict(linearisation='operator'), dict(linearisation='full', parameter='rho')):
        host = prob.Hvec(None, p, u=[F[0]], resid=r, **kw)
        for H in (prob.Hvec(None, p, u=F, resid=r, **kw), prob.Hvec(None, p, resid=r, **kw)):
            assert rel(H, host) <= 1e-6
    F.release()
    del prob.factors


# ---- 4. central differences of the device gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lin,par', [('full', 'c'), ('operator', 'rho'), ('operator', 'c')])
def test_central_differences_of_the_device_gradient_converge_to_the_device_hvec(helm_lib, monkeypatch, lin, par):
    """test 2 of test_newton_host.py through the device routes: dpred, Jtvec and Hvec(resid=) all with the fields in HBM.  'operator' with 'c': the perturbation
    vanishes in the absorbing layers and the cells outside them are compared."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = xc.pair('fixed', False, device=True, rtol=1e-11)
    c0, rho0 = fc.model()
    dobs = nc.observed(prob, sv, c0)
    kw = dict(linearisation=lin, parameter=par)
    layers = lin == 'operator' and par == 'c'
    p = dc.perturbation() if par == 'rho' else (nc.outside_layers() if layers else nc.everywhere())
    keep = (p != 0) if layers else None
    F = prob.fieldsDevice(c0)
    r = sv.dpred(None, u=F) - dobs
    Hp, Hgn = prob.Hvec(None, p, u=F, resid=r, **kw), prob.Hvec(None, p, u=F, **kw)
    F.release()
    g = nc.gradient_of(prob, sv, dobs, **kw)
    rn = nc.central_remainders(g, rho0 if par == 'rho' else c0, p, Hp, keep)
    print('device %s %s: remainders %s factors %s; ||Hp - JtJp|| / ||Hp|| = %.3f' % (lin, par, rn, fc.factors(rn), fc.norm(Hp - Hgn) / fc.norm(Hp)))
    assert all(f >= nc.SECOND for f in fc.factors(rn))
    del prob.factors


# ---- 5. the routes that were there are what they were ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', sorted(xc.RECORDED_MODES))
def test_the_recorded_products_are_reproduced_bit_for_bit(helm_lib, monkeypatch, mode):
    "tests/golden/g13_operator_device.npz through full_cases.recorded_products: JvecBorn, Jtvec and the Gauss-Newton Hvec (resid=None) as they were recorded"
    monkeypatch.setenv('HELM_DEVICES', '0')
    gold = np.load(xc.RECORDING)
    now = xc.recorded_products(mode)
    for key, val in now.items():
        want = gold['%s/%s' % (mode, key)]
        assert val.dtype == want.dtype and val.shape == want.shape, key
        assert np.array_equal(bits(val), bits(want)), (key, rel(val, want))
