"""GPU: the buoyancy derivative of the 3-D operator on the device -- the kernels of csrc/survey3d_density.hip against 80-bit references with bounds counted from
their rounded operations (tests/survey3d_density_cases.py), and the routes derivatives3D=True opens on Helm3DProblem against the host maps of frechet3d.py."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import survey3d_cases as s3
from tests import survey3d_density_cases as d3c
from tests.test_gpu_survey3d import ROUTE_DIMS, bits, lu_of, route_config

pytestmark = pytest.mark.gpu

GRIDS = [(5, 6, 7), (4, 9, 66), (7, 4, 64), (3, 3, 3), (6, 5, 130)]          # (nz, ny, nx): x below, at and past the 64-wide tile, y not a multiple of 4
T = dict(adjoint='transpose')


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _worst(err, bound):
    ok = bound > 0
    assert np.all(err[~ok] == 0)
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---- 6. the kernels against 80-bit evaluations ----------------------------------------------------------------------------------------------------------
def check_lap_kernels(op, dims, k, seed, conjs=(True, False), imaging=True):
    import torch
    from zephyr_amd import device_survey3d as d3
    N = op.nrow
    ld = N + 5                                                # a leading dimension past N: the padding must stay untouched
    rng = np.random.default_rng(seed)
    U, B, R0 = s3.randc(rng, (k, ld)), rng.uniform(-1., 2., N), s3.randc(rng, (k, ld))
    coef = complex(0.7, -1.3)
    inside = s3._interior(dims).ravel()
    dU, dB = _dev(U), _dev(B)
    worst = {}
    for conj in conjs:
        for add in (False, True):
            ref, bound = d3c.lap_sources_reference(op, U[:, :N], B, coef, conj, R0[:, :N] if add else None)
            outs = []
            for _ in range(2):
                R = _dev(R0) if add else torch.full((k, ld), 7.0 + 0j, dtype=torch.complex128, device='cuda:0')
                torch.cuda.synchronize()
                d3.lapSourcesDevice(op, dU, k, dB, coef, R, conj=conj, add=add, ldu=ld, ldr=ld)
                outs.append(R.cpu().numpy())
            got = outs[0]
            assert np.array_equal(bits(outs[1]), bits(got))                      # repeated launches: the same bits
            assert np.array_equal(bits(got[:, N:]), bits(R0[:, N:] if add else np.full((k, ld - N), 7.0 + 0j)))          # nothing written past N
            if add:
                assert np.array_equal(bits(got[:, :N][:, ~inside]), bits(R0[:, :N][:, ~inside]))                         # the boundary rows are left alone
            else:
                assert np.all(bits(got[:, :N][:, ~inside]) == 0)                                                         # ... or exact zeros (+0.0)
            worst['sources conj=%d add=%d' % (conj, add)] = _worst(np.abs(got[:, :N].astype(np.clongdouble) - ref), bound)
    # imaging: accumulation into a non-zero P, the boundary rows of UB poisoned
    if not imaging:
        print('%s k=%d: worst error / bound %s' % (dims, k, {n: '%.3f' % v for n, v in worst.items()}))
        assert max(worst.values()) <= 1.0, worst
        return
    UF, UB, P0 = s3.randc(rng, (k, ld)), s3.randc(rng, (k, ld)), s3.randc(rng, N)
    UB[:, :N][:, ~inside] = 1e300 * (1 + 1j)
    dF, dZ = _dev(UF), _dev(UB)
    for conj in (False, True):
        ref, bound = d3c.lap_imaging_reference(op, UF[:, :N], UB[:, :N], P0, conj)
        outs = []
        for _ in range(2):
            P = _dev(P0)
            torch.cuda.synchronize()
            d3.lapImagingAccumulateDevice(op, dF, dZ, k, P, conj=conj, ldf=ld, ldb=ld)
            outs.append(P.cpu().numpy())
        assert np.all(np.isfinite(outs[0].view(np.float64)))      # the mask holds: 1e300 never entered a product
        assert np.array_equal(bits(outs[0]), bits(outs[1]))
        worst['imaging conj=%d' % conj] = _worst(np.abs(outs[0].astype(np.clongdouble) - ref), bound)
    print('%s k=%d: worst error / bound %s' % (dims, k, {n: '%.3f' % v for n, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('dims', GRIDS, ids=lambda d: 'x'.join(map(str, d)))
def test_lap_kernels_against_extended_precision(helm_lib, dims, k):
    import zephyr_amd as za
    op = za.Helm3D(d3c.small_config(dims, seed=k))
    check_lap_kernels(op, dims, k, 100 * k + sum(dims))
    del op.factors


def test_lap_sources_column_loop_runs_three_rounds(helm_lib):
    """(6, 5, 130) has 36 tiles, so the sources kernel spreads the columns over min(57, k) workgroups along grid.y: with 3 x 57 + 2 = 173 columns every
    workgroup walks at least three columns -- the first two four --, and the double buffer of the in-workgroup loop goes round"""
    import zephyr_amd as za
    dims = (6, 5, 130)
    op = za.Helm3D(d3c.small_config(dims, seed=5))
    check_lap_kernels(op, dims, 173, 77, conjs=(True,), imaging=False)
    del op.factors


def test_buoyancy_chain_kernel_and_refusals(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib, frechet3d
    from zephyr_amd import device_survey3d as d3
    dims = (6, 5, 70)
    cfg = d3c.small_config(dims, seed=9)
    op = za.Helm3D(cfg)
    N = op.nrow
    rng = np.random.default_rng(2)
    din, Pl, Pm, G0 = rng.standard_normal(N), s3.randc(rng, N), s3.randc(rng, N), rng.standard_normal(N)
    din[::7] *= 1e-9                                          # cells of every size side by side: each is held to its own majorant
    Pl[::5] *= 1e-7
    Pm[1::5] *= 1e6
    G0[::3] *= 1e-8
    w = complex(0.4, -0.9)
    worst = {}
    for gardner in (0, 1):                                    # (Gardner's d b / d c with the handle's b = 1 / rho)
        W, DB = torch.zeros(N, dtype=torch.complex128, device='cuda:0'), torch.zeros(N, dtype=torch.float64, device='cuda:0')
        G = _dev(G0)
        dIn, dPl, dPm = _dev(din), _dev(Pl), _dev(Pm)
        torch.cuda.synchronize()
        d3.buoyChainDevice(op, gardner, dIn, None, None, w, DB, W)
        d3.buoyChainDevice(op, gardner, None, dPl, dPm, w, None, G)
        ref = d3c.buoy_chain_reference(op, gardner, din, Pl, Pm, G0, w)
        got = dict(DB=DB.cpu().numpy().astype(np.longdouble), W=W.cpu().numpy().astype(np.clongdouble), G=G.cpu().numpy().astype(np.longdouble))
        for name, (want, bound) in ref.items():
            worst['%s gardner=%d' % (name, gardner)] = _worst(np.abs(got[name] - want), bound)
    # the Gardner chain of a handle whose density IS the default one is that of b = Re(c)^-0.25 / 310
    og = za.Helm3D({k_: v_ for k_, v_ in dict(cfg, c=np.asarray(cfg['c']).real).items() if k_ != 'rho'})
    DB = torch.zeros(N, dtype=torch.float64, device='cuda:0')
    W = torch.zeros(N, dtype=torch.complex128, device='cuda:0')
    d3.buoyChainDevice(og, 1, _dev(din), None, None, w, DB, W)
    want, bound = d3c.gardner_db_reference(og, din)
    worst['DB default density'] = _worst(np.abs(DB.cpu().numpy().astype(np.longdouble) - want), bound)
    print('k_buoy3_chain %s: worst error / bound %s' % (dims, {n: '%.3f' % v for n, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    assert np.abs(frechet3d.gardnerChain3(og) * din - want.astype(np.float64)).max() <= 8 * s3.U53 * np.abs(want).max()      # (and frechet3d's chain is that one)
    # a 2-D handle is refused by all three
    mz = za.MiniZephyr(dict(nx=20, nz=24, dx=10., c=2500., freq=10., nPML=5))
    buf = torch.zeros(4 * 480, dtype=torch.complex128, device='cuda:0')
    p, p2 = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 16 * 960)
    assert helm_lib.helm_lap3_sources_device(mz.handle, p, 1, 480, p, 1.0, 0.0, 0, 0, p2, 480) == -4
    assert '3-D' in _lib.last_error(mz.handle)
    assert helm_lib.helm_lap3_imaging_accumulate_device(mz.handle, p, 480, p, 480, 1, 0, p2) == -4
    assert helm_lib.helm_buoy3_chain_device(mz.handle, 0, p, None, None, 1.0, 0.0, p2, ctypes.c_void_p(buf.data_ptr() + 16 * 1920)) == -4
    # overlapping, short or misaligned arguments on a 3-D handle
    big = torch.zeros(4 * N, dtype=torch.complex128, device='cuda:0')
    b = big.data_ptr()
    P_ = lambda off: ctypes.c_void_p(b + off)
    assert helm_lib.helm_lap3_sources_device(op.handle, P_(0), 1, N, P_(16 * N), 1.0, 0.0, 0, 0, P_(0), N) == -1                     # R over U
    assert helm_lib.helm_lap3_sources_device(op.handle, P_(0), 1, N, P_(32 * N), 1.0, 0.0, 0, 1, P_(32 * N), N) == -1                # R over B
    assert helm_lib.helm_lap3_sources_device(op.handle, P_(0), 1, N - 1, P_(16 * N), 1.0, 0.0, 0, 0, P_(32 * N), N) == -1            # ldu < N
    assert helm_lib.helm_lap3_sources_device(op.handle, P_(8), 1, N, P_(16 * N), 1.0, 0.0, 0, 0, P_(32 * N), N) == -1                # U misaligned
    assert helm_lib.helm_lap3_imaging_accumulate_device(op.handle, P_(0), N, P_(16 * N), N, 1, 0, P_(16 * N)) == -1                  # P over UB
    assert helm_lib.helm_lap3_imaging_accumulate_device(op.handle, P_(0), N, P_(16 * N), N - 1, 1, 0, P_(32 * N)) == -1              # ldb < N
    assert helm_lib.helm_lap3_imaging_accumulate_device(op.handle, P_(0), N, P_(16 * N), N, 0, 0, P_(32 * N)) == -1                  # no columns
    assert helm_lib.helm_buoy3_chain_device(op.handle, 0, P_(0), None, None, 1.0, 0.0, P_(16 * N), P_(0)) == -1                      # out over the input
    assert helm_lib.helm_buoy3_chain_device(op.handle, 0, P_(0), None, None, 1.0, 0.0, P_(0), P_(16 * N)) == -1                      # db over the input
    assert helm_lib.helm_buoy3_chain_device(op.handle, 0, None, P_(0), None, 1.0, 0.0, None, P_(32 * N)) == -1                       # a plane missing
    assert helm_lib.helm_buoy3_chain_device(op.handle, 0, None, P_(0), P_(16 * N), 1.0, 0.0, None, P_(4)) == -1                      # G misaligned
    # a handle that is not assembled
    raw = helm_lib.helm_create3d(0, 6, 5, 70, 9., 11., 10., 2)
    try:
        assert helm_lib.helm_lap3_sources_device(raw, P_(0), 1, N, P_(16 * N), 1.0, 0.0, 0, 0, P_(32 * N), N) == -3
        assert 'not assembled' in _lib.last_error(raw)
        assert helm_lib.helm_lap3_imaging_accumulate_device(raw, P_(0), N, P_(16 * N), N, 1, 0, P_(32 * N)) == -3
        assert helm_lib.helm_buoy3_chain_device(raw, 0, None, P_(0), P_(16 * N), 1.0, 0.0, None, P_(32 * N)) == -3
    finally:
        helm_lib.helm_destroy(raw)
    del op.factors, og.factors, mz.factors


# ---- 7. the routes ----------------------------------------------------------------------------------------------------------------------------------------
_ROUTES = {}


def device_pair(mode, gardner=False, **extra):
    import zephyr_amd as za
    sc = dict(route_config(mode), derivatives3D=True, **extra)
    if gardner:
        del sc['rho']
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def routes(mode, gardner=False):
    'one device pair per receiver mode and density convention for the module, with its stored fields and inputs'
    if (mode, gardner) not in _ROUTES:
        prob, sv = device_pair(mode, gardner)
        rng = np.random.default_rng(11)
        _ROUTES[(mode, gardner)] = dict(prob=prob, sv=sv, F=prob.fieldsDevice(), r=s3.randc(rng, sv.nD), v=rng.standard_normal(2 * prob.nrow))
    return _ROUTES[(mode, gardner)]


def kinds(mode):
    "(label, routes entry, keywords, size of v)"
    N = int(np.prod(ROUTE_DIMS))
    return [('rho', routes(mode), dict(linearisation='operator', parameter='rho'), N), ('joint', routes(mode), dict(linearisation='full', parameter='joint'), 2 * N),
            ('gardner', routes(mode, True), dict(linearisation='full', parameter='c'), N)]


def kind(mode, label):
    return next(x for x in kinds(mode) if x[0] == label)


def host_gradient(prob, Fh, caught, parameter, gardner):
    'the host maps of frechet3d.py on downloaded fields: what Helm3DProblem.Jtvec forms without a GPU'
    from zephyr_amd import frechet3d
    N, st = prob.nrow, complex(prob.system.scaleTerm)
    g = np.zeros(2 * N if parameter == 'joint' else N)
    gb = g[N:] if parameter == 'joint' else g
    M = frechet3d.massStencil3(ROUTE_DIMS)
    for i, UB in enumerate(caught):
        op = prob.system.subProblems[i]
        uh, lam, w = np.conj(Fh[i] / st), np.conj(UB), -np.conj(st) / complex(op.premul)
        if gardner or parameter in ('c', 'joint'):
            g[:N] += (w * frechet3d.velocityChain3(op) * frechet3d.imagingSum3(op, uh, lam, M)).real
        if gardner or parameter in ('rho', 'joint'):
            chain = frechet3d.gardnerChain3(op) if gardner else frechet3d.densityChain3(op)
            gb += chain * (w * frechet3d.buoyancyImaging3(op, uh, lam, frechet3d.lapStencil3(op), M)).real
    return g


def host_born_sources(prob, Fh, v, parameter, gardner):
    from zephyr_amd import frechet3d
    N, st = prob.nrow, complex(prob.system.scaleTerm)
    M = frechet3d.massStencil3(ROUTE_DIMS)
    out = []
    for i, op in enumerate(prob.system.subProblems):
        uh = np.conj(Fh[i] / st)
        q = 0.0
        if gardner or parameter in ('c', 'joint'):
            q = q + frechet3d.bornSources3(op, v[:N], uh, M)
        if gardner or parameter in ('rho', 'joint'):
            chain = frechet3d.gardnerChain3(op) if gardner else frechet3d.densityChain3(op)
            q = q + frechet3d.buoyancySources3(op, chain * v[-N:], uh, frechet3d.lapStencil3(op), M)
        out.append(q / -complex(op.premul))
    return out


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_maps_on_the_same_fields(helm_lib, monkeypatch, mode):
    """device Jtvec / JvecBorn fed the stored F against the host maps fed the DOWNLOADED F and the downloaded back-propagated fields (caught where the device
    route hands them to the imaging kernel); the adjoint identity on the device"""
    from zephyr_amd import _lib
    from zephyr_amd import device_survey3d as d3
    for label, R_, kw, n in kinds(mode):
        prob, sv, F, r, v = R_['prob'], R_['sv'], R_['F'], R_['r'], R_['v'][:n]
        gardner = label == 'gardner'
        assert prob._deviceGradientAvailable()
        Fh = [F[i] for i in range(sv.nfreq)]
        caught, born = [], []
        real_imaging, real_sources = d3.lapImagingAccumulateDevice, d3.lapSourcesDevice

        def imaging(op, d_uf, d_ub, nsrc, d_p, **k_):
            caught.append(np.array(_lib.from_device(d_ub).reshape((nsrc, -1)).T))
            return real_imaging(op, d_uf, d_ub, nsrc, d_p, **k_)

        def sources(op, d_u, nsrc, d_b, coef, d_r, **k_):
            out = real_sources(op, d_u, nsrc, d_b, coef, d_r, **k_)
            born.append(np.array(_lib.from_device(d_r).reshape((nsrc, -1)).T))          # (the complete right-hand side: the kappa part is in it already)
            return out
        monkeypatch.setattr(d3, 'lapImagingAccumulateDevice', imaging)
        g = prob.Jtvec(None, r, u=F, **T, **kw)
        monkeypatch.setattr(d3, 'lapImagingAccumulateDevice', real_imaging)
        monkeypatch.setattr(d3, 'lapSourcesDevice', sources)
        J = prob.JvecBorn(None, v, u=F, **kw)
        monkeypatch.setattr(d3, 'lapSourcesDevice', real_sources)
        assert g.dtype == np.float64 and g.shape == (n,) and len(caught) == sv.nfreq and len(born) == sv.nfreq
        e_g = s3.rel(g, host_gradient(prob, Fh, caught, kw['parameter'], gardner))
        e_q = max(s3.rel(b_, q_) for b_, q_ in zip(born, host_born_sources(prob, Fh, v, kw['parameter'], gardner)))
        lhs, rhs = s3.inner(r, J), float(g @ v)
        print('%s %s: device gradient against the host maps on the same fields %.2e, Born sources %.2e; adjoint identity on the device misses by %.2e'
              % (mode, label, e_g, e_q, abs(lhs - rhs) / abs(lhs)))
        assert e_g <= 1e-12 and e_q <= 1e-12
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
        # repeated calls on the same stored fields give the same bits
        assert np.array_equal(bits(prob.Jtvec(None, r, u=F, **T, **kw)), bits(g)) and np.array_equal(bits(prob.JvecBorn(None, v, u=F, **kw)), bits(J))
        if label == 'joint':                  # the two halves of the joint gradient are the single-parameter gradients (one back-solve against two)
            N = prob.nrow
            O = dict(linearisation='full')
            assert s3.rel(g[:N], prob.Jtvec(None, r, u=F, **T, **O)) <= 1e-6 and s3.rel(g[N:], prob.Jtvec(None, r, u=F, **T, **O, parameter='rho')) <= 1e-6
            Hv = prob.Hvec(None, v, u=F, **kw)
            assert Hv.shape == (2 * N,) and s3.rel(Hv, prob.Jtvec(None, J, u=F, **T, **kw)) <= 1e-6 and float(Hv @ v) > 0


class OracleOnLU(s3.OracleHelm3D):
    "the stand-in with the module's shared factors (those of tests/test_gpu_survey3d.py: the model is the same): A^-T from the LU of A"
    LU_TAG = 'route'

    def __mul__(self, rhs):
        if sp.issparse(rhs):
            rhs = rhs.toarray()
        lu = lu_of((self.LU_TAG, complex(self.freq)), lambda: s3.oracle_matrix(self))
        x = lu.solve(complex(self.premul) * np.asarray(rhs, dtype=np.complex128), trans='T' if self.transposed else 'N')
        return np.conj(x)


class OracleOnLUT(OracleOnLU, s3.OracleHelm3DT):
    'A^-T from the same factors'


OracleOnLU.Transposed = OracleOnLUT


class GardnerOnLU(OracleOnLU):
    'the same for the config without `rho`: another matrix, factors of its own'
    LU_TAG = 'route-gardner'


class GardnerOnLUT(GardnerOnLU, s3.OracleHelm3DT):
    'A^-T from the same factors'


GardnerOnLU.Transposed = GardnerOnLUT


@pytest.mark.parametrize('mode,label', [('fixed', 'rho'), ('fixed', 'joint'), ('fixed', 'gardner'), ('relative', 'rho'), ('relative', 'joint'),
                                        ('relative', 'gardner')])
def test_device_routes_end_to_end_against_the_sparse_lu(helm_lib, mode, label):
    """gradient and Born data at rtol = 1e-9 against the host route on splu: 1e-5 allows two fields of 1e-6 each multiplied together and the second solve.  (The
    Gardner matrix is another one: its two factorisations, 4 s each, are made by the first Gardner case and shared with the second.)"""
    import zephyr_amd as za
    _, R_, kw, n = kind(mode, label)
    prob, sv, F, r, v = R_['prob'], R_['sv'], R_['F'], R_['r'], R_['v'][:n]
    sc = dict(route_config(mode), Disc=GardnerOnLU if label == 'gardner' else OracleOnLU, hostGradient=True, derivatives3D=True)
    if label == 'gardner':
        del sc['rho']
    hp, hs = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    hp.pair(hs)
    g, J = prob.Jtvec(None, r, u=F, **T, **kw), prob.JvecBorn(None, v, u=F, **kw)
    Fhost = hp.fields(None)
    gh, Jh = hp.Jtvec(None, r, u=Fhost, **T, **kw), hp.JvecBorn(None, v, u=Fhost, **kw)
    e = dict(gradient=s3.rel(g, gh), born=s3.rel(J, Jh))
    print('%s %s: device routes against the host route on splu %s' % (mode, label, {k_: '%.2e' % x for k_, x in e.items()}))
    assert e['gradient'] <= 1e-5 and e['born'] <= 1e-5


@pytest.mark.parametrize('label', ['rho', 'joint', 'gardner'])
def test_taylor_remainders_through_the_device_routes(helm_lib, label):
    _, R_, kw, n = kind('fixed', label)
    prob, sv, F = R_['prob'], R_['sv'], R_['F']
    c0 = np.array(prob.systemConfig['c'])
    N = prob.nrow
    rng = np.random.default_rng(21)
    u_ = rng.uniform(0.3, 1., 2 * N) * rng.choice([-1., 1.], 2 * N)
    dc, dr = 120. * u_[:N].reshape(c0.shape), 100. * u_[N:].reshape(c0.shape)
    if label == 'gardner':
        v, moved = dc.ravel(), lambda h: c0 + h * dc
    else:
        rho0 = np.array(prob.systemConfig['rho'])
        v = dr.ravel() if label == 'rho' else np.concatenate([dc.ravel(), dr.ravel()])
        moved = (lambda h: dict(c=c0, rho=rho0 + h * dr)) if label == 'rho' else (lambda h: dict(c=c0 + h * dc, rho=rho0 + h * dr))
    d0 = sv.dpred(None, u=F)
    J = prob.JvecBorn(None, v, u=F, **kw)
    p2, s2 = device_pair('fixed', gardner=label == 'gardner')
    rem = [np.linalg.norm(s2.dpred(moved(0.5 ** j)) - d0 - 0.5 ** j * J) for j in range(4)]
    ratios = [rem[j] / rem[j + 1] for j in range(3)]
    print('%s: Taylor remainders through the device routes %s, ratios %s, rtol |d| = %.1e' % (label, ['%.3e' % x for x in rem], ['%.3f' % x for x in ratios],
                                                                                          1e-9 * np.linalg.norm(d0)))
    assert rem[-1] >= 100 * 1e-9 * np.linalg.norm(d0)          # the smallest remainder stays 100 x above the solver's tolerance
    assert all(3.8 <= x <= 4.2 for x in ratios), (label, ratios)
    del p2.factors


# ---- 8. the velocity route is what it was ---------------------------------------------------------------------------------------------------------------
def test_velocity_route_is_bit_identical_with_and_without_the_key(helm_lib):
    """parameter='c' with an explicit rho runs the launches it ran before the key existed: the same bits with and without it, with u=None and with u=F.
    Compared on fresh pairs, so that every solve has the same history on both sides (a used 3-D handle does not repeat a solve to the bit)."""
    from tests.test_gpu_survey3d import device_pair as plain_pair
    rng = np.random.default_rng(11)
    X = dict(adjoint='transpose', linearisation='operator')
    out = []
    for make, stored in ((plain_pair, True), (device_pair, True), (device_pair, False)):
        pg, sg = make('relative')
        pb, sb = make('relative')
        if not out:
            r, v = s3.randc(rng, sg.nD), rng.standard_normal(pg.nrow)
        Fg, Fb = (pg.fieldsDevice(), pb.fieldsDevice()) if stored else (None, None)
        out.append((pg.Jtvec(None, r, u=Fg, **X), pb.JvecBorn(None, v, u=Fb, linearisation='operator')))
        del pg.factors, pb.factors
    print('with the key against without: gradient %.2e, Born data %.2e; u=None against u=F: %.2e, %.2e'
          % (s3.rel(out[1][0], out[0][0]), s3.rel(out[1][1], out[0][1]), s3.rel(out[2][0], out[1][0]), s3.rel(out[2][1], out[1][1])))
    for a in (1, 2):
        assert np.array_equal(bits(out[a][0]), bits(out[0][0])) and np.array_equal(bits(out[a][1]), bits(out[0][1]))


def test_joint_u_none_is_bit_identical_to_the_stored_fields(helm_lib):
    rng = np.random.default_rng(11)
    kw = dict(linearisation='full', parameter='joint')
    out = []
    for stored in (False, True):
        pg, sg = device_pair('relative')
        pb, sb = device_pair('relative')
        if not out:
            r, v = s3.randc(rng, sg.nD), rng.standard_normal(2 * pg.nrow)
        Fg, Fb = (pg.fieldsDevice(), pb.fieldsDevice()) if stored else (None, None)
        out.append((pg.Jtvec(None, r, u=Fg, **T, **kw), pb.JvecBorn(None, v, u=Fb, **kw)))
        del pg.factors, pb.factors
    print('joint, u=None against u=F on fresh pairs: gradient %.2e, Born data %.2e' % (s3.rel(out[0][0], out[1][0]), s3.rel(out[0][1], out[1][1])))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))


# ---- 9. ranks -----------------------------------------------------------------------------------------------------------------------------------------------
RANKS = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
os.environ['HELM_DEVICES'] = '0'
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import survey3d_cases as s3
from tests.test_gpu_survey3d_density import device_pair
ref, sref = device_pair('relative', shardFreqs=False)
prob, sv = device_pair('relative')
assert prob._deviceGradientAvailable() and prob.ownedFreqs == [dist.get_rank()] and ref.ownedFreqs == [0, 1]
rng = np.random.default_rng(11)
r, v = s3.randc(rng, sv.nD), rng.standard_normal(2 * prob.nrow)
F = prob.fieldsDevice()
kw = dict(linearisation='full', parameter='joint')
# the gradient to 1e-12 (its solves have the same history on both sides and come out the same to the bit); the Born data re-solve on handles that have
# solved before, and two solves of one system at rtol = 1e-9 agree to the suite's 3-D tolerance at this rtol, 1e-6
g = prob.Jtvec(None, r, u=F, adjoint='transpose', **kw)
e = [s3.rel(g, ref.Jtvec(None, r, adjoint='transpose', **kw)), s3.rel(prob.JvecBorn(None, v, u=F, **kw), ref.JvecBorn(None, v, **kw))]
print('RANK', dist.get_rank(), ['%%.2e' %% x for x in e], flush=True)
ok = g.shape == (2 * prob.nrow,) and e[0] <= 1e-12 and e[1] <= 1e-6
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_joint_gradient(helm_lib, tmp_path):
    "the two frequencies sharded over two ranks on one GPU: ONE all-reduce of the (2 N,) vector gives every rank the single-rank joint gradient"
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'ranks.py'
    script.write_text(RANKS % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29673', WORLD_SIZE='2', PYTHONPATH=root)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    try:
        outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        print(o)
        assert p.returncode == 0 and ('RANK %d OK' % r) in o, o
