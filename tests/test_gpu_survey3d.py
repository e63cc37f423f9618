"""GPU: the 3-D survey layer on the device -- the transposed 27 planes (a permutation, bit for bit), the transposed solve through both multigrid set-ups, the
two mass-stencil kernels of csrc/survey3d.hip against 80-bit references with bounds counted from their rounded operations, and the device routes of
Helm3DProblem against the host maps (tests/survey3d_cases.py has the stand-in operator, the references and the surveys)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import helm3d_oracle as h3
from tests import survey3d_cases as s3

pytestmark = pytest.mark.gpu

GRIDS = [(5, 6, 7), (4, 9, 66), (7, 4, 64), (3, 3, 3), (6, 5, 130)]          # (nz, ny, nx): x below, at and past the 64-wide tile, y not a multiple of 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def small_config(dims, seed=0):
    'a heterogeneous model with complex c, dx != dy != dz and a finite tau on a small grid'
    nz, ny, nx = dims
    rng = np.random.default_rng(seed)
    c = (1800. + 1500. * rng.random(dims)) * (1 + 0.01j)
    rho = 1000. + 500. * rng.random(dims)
    return dict(nx=nx, ny=ny, nz=nz, dx=9., dy=11., dz=10., c=c, rho=rho, freq=11., tau=0.5, nPML=2, cPML=250.)


def planes_to_csr(C):
    return h3.coefficients_to_csr3(C)


# ---- 1. the transposed planes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', GRIDS, ids=lambda d: 'x'.join(map(str, d)))
def test_transposed_planes_are_a_permutation_bit_for_bit(helm_lib, dims):
    import zephyr_amd as za
    from zephyr_amd import _lib
    cfg = small_config(dims, seed=sum(dims))
    plain, tr = za.Helm3D(cfg), za.Helm3DTransposed(cfg)
    C, CT = plain.diagonals(), tr.diagonals()
    assert helm_lib.helm_get_transposed(tr.handle) == 1 and helm_lib.helm_get_transposed(plain.handle) == 0
    assert np.array_equal(bits(CT), bits(s3.transpose_planes3(C)))
    A, AT = plain.A, tr.A
    D = sp.csr_matrix(A.T) - AT
    assert D.nnz == 0 or abs(D).max() == 0
    assert A.nnz == AT.nnz
    # back to the plain planes: in force from the next assembly only
    h = tr.handle
    f = complex(tr.freq)
    assert helm_lib.helm_set_transposed(plain.handle, 1) == -4        # (the 2-D entry point refuses a 3-D handle, as it did)
    _lib.check(helm_lib.helm_set_transposed3d(h, 0), h)
    assert helm_lib.helm_get_transposed(h) == 1
    _lib.check(helm_lib.helm_assemble(h, f.real, f.imag, float(tr.tau), 0.0, float(tr.cPML)), h)
    assert helm_lib.helm_get_transposed(h) == 0
    assert np.array_equal(bits(tr.diagonals()), bits(C))
    # and the apply of a transposed handle is A^T x, from stored planes
    tr2 = za.Helm3DTransposed(cfg)
    rng = np.random.default_rng(1)
    X = s3.randc(rng, (plain.nrow, 5))
    ref = A.T @ X
    assert np.abs(tr2.applyForward(X) - ref).max() <= 1e-13 * np.abs(ref).max()
    del plain.factors, tr.factors, tr2.factors


# ---- 2. the transposed solve ------------------------------------------------------------------------------------------------------------------------
_LU = {}


def lu_of(key, make):
    'one sparse LU per model for the whole module (4 s each at these sizes with this ordering, 8 s with the default): A^-T comes from the same factors, solve(trans=\'T\')'
    if key not in _LU:
        _LU[key] = spla.splu(make().tocsc(), permc_spec='MMD_ATA')
    return _LU[key]


def random_model():
    nz, ny, nx = 30, 26, 28
    rng = np.random.default_rng(3)
    c = 1900. + 400. * rng.random((nz, ny, nx))
    rho = 1000. + 100. * rng.random((nz, ny, nx))
    return dict(nx=nx, ny=ny, nz=nz, dx=10., c=c, rho=rho, freq=6., nPML=6, rtol=1e-9, maxit=20000)


def layered_model():
    nz, ny, nx = 30, 32, 28
    iz = np.arange(nz)[:, None, None]
    c = (1800. + 25. * iz + 150. * (iz > 18)) * np.ones((nz, ny, nx))
    rho = 1000. + 300. * (iz > 18) * np.ones((nz, ny, nx))
    return dict(nx=nx, ny=ny, nz=nz, dx=10., c=c, rho=rho, freq=4., nPML=6, rtol=1e-9, maxit=20000)


def point_sources(cfg, n):
    nz, ny, nx = cfg['nz'], cfg['ny'], cfg['nx']
    q = np.zeros((nz * ny * nx, n), complex)
    rng = np.random.default_rng(n)
    for s in range(n):
        iz, iy, ix = (int(rng.integers(2 if s % 3 else 8, d - 2)) for d in (nz, ny, nx))      # (every third one may lie inside the absorbing layers)
        q[(iz * ny + iy) * nx + ix, s] = 1.0 + 0.1j * s
    return q


def solve_both(cfg, q, label):
    'the transposed and the plain solve of one case: checks the transposed one against the sparse LU and returns both iteration counts'
    import zephyr_amd as za
    lu = lu_of((cfg['nz'], cfg['ny'], cfg['nx'], cfg['freq']),
               lambda: h3.coefficients_to_csr3(h3.helm3d_coefficients(cfg['nz'], cfg['ny'], cfg['nx'], cfg['c'], cfg['rho'], cfg['freq'], dx=10., nPML=6)))
    ref_t = np.conj(lu.solve(q, trans='T'))
    op, op_t = za.Helm3D(cfg), za.Helm3DTransposed(cfg)
    u = op * q
    u_t = op_t * q
    its, its_t = (max(i['iterations'] for i in o.lastInfo) for o in (op, op_t))
    err = s3.rel(u_t, ref_t)
    print('%s: iterations transposed %d, plain %d; transposed solve against the sparse LU %.2e (plain %.2e)' % (label, its_t, its, err, s3.rel(u, np.conj(lu.solve(q)))))
    assert all(i['status'] == 0 for i in op_t.lastInfo), op_t.lastInfo
    assert err <= 1e-6
    assert s3.rel(u_t, u) > 1e-2                        # (it IS another operator: the fields differ)
    assert its_t <= 2 * its, (its_t, its)
    info = [dict(i) for i in op_t.lastInfo]
    del op.factors, op_t.factors
    return info


@pytest.mark.parametrize('method', ['mg', 'bicgstab'])
def test_transposed_solve_random_model(helm_lib, method):
    cfg = dict(random_model(), method=method)
    solve_both(cfg, point_sources(cfg, 2), 'random 30x26x28, 6 Hz, %s' % method)


@pytest.mark.parametrize('keep', ['1', '0'])
def test_transposed_solve_layered_model_both_hierarchies(helm_lib, monkeypatch, keep):
    "the layered model takes the layer-preserving hierarchy (Galerkin levels, direct coarse solve); HELM_MG3_KEEP=0: the standard shifted cycle"
    monkeypatch.setenv('HELM_MG3_KEEP', keep)
    cfg = dict(layered_model(), method='mg')
    q = point_sources(cfg, 3)
    q[(22 * 32 + 27) * 28 + 4, 2] = 2.0j                 # inside the absorbing layers
    solve_both(cfg, q, 'layered 30x32x28, 4 Hz, HELM_MG3_KEEP=%s' % keep)


def test_transposed_solve_batch_of_17(helm_lib):
    cfg = dict(random_model(), method='mg', batch=17)
    solve_both(cfg, point_sources(cfg, 17), 'random 30x26x28, 6 Hz, mg, 17 right-hand sides')


def test_plain_operator_is_untouched_by_a_transposed_neighbour(helm_lib):
    "the untransposed operator gives the same bits before and after a transposed handle has lived on the device"
    import zephyr_amd as za
    cfg = dict(random_model(), method='mg')
    q = point_sources(cfg, 4)
    op = za.Helm3D(cfg)
    u0, C0 = op * q, op.diagonals()
    its0 = [i['iterations'] for i in op.lastInfo]
    del op.factors
    t = za.Helm3DTransposed(cfg)
    t * q
    op = za.Helm3D(cfg)
    u1 = op * q
    assert np.array_equal(bits(u1), bits(u0)) and np.array_equal(bits(op.diagonals()), bits(C0)) and [i['iterations'] for i in op.lastInfo] == its0
    del t.factors
    u2 = op * q
    assert np.array_equal(bits(u2), bits(u0))
    del op.factors


# ---- 3. the kernels against 80-bit evaluations ------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


@pytest.mark.parametrize('k', [1, 3, 17])
@pytest.mark.parametrize('dims', GRIDS, ids=lambda d: 'x'.join(map(str, d)))
def test_mass_kernels_against_extended_precision(helm_lib, dims, k):
    import torch
    import zephyr_amd as za
    from zephyr_amd import device_survey3d as d3
    op = za.Helm3D(small_config(dims, seed=k))
    N = op.nrow
    ld = N + 5                                                # a leading dimension past N: the padding must stay untouched
    rng = np.random.default_rng(100 * k + sum(dims))
    U, W = s3.randc(rng, (k, ld)), s3.randc(rng, N)
    coef = complex(0.7, -1.3)
    inside = s3._interior(dims).ravel()
    worst = {}
    for conj in (True, False):
        ref, bound = s3.mass_sources_reference(dims, U[:, :N], W, coef, conj)
        R = torch.full((k, ld), 7.0 + 0j, dtype=torch.complex128, device='cuda:0')
        dU, dW = _dev(U), _dev(W)
        torch.cuda.synchronize()
        d3.massSourcesDevice(op, dU, k, dW, coef, R, conj=conj, ldu=ld, ldr=ld)
        got = R.cpu().numpy()
        assert np.all(got[:, N:] == 7.0)                      # nothing written past N
        assert np.all(bits(got[:, :N][:, ~inside]) == 0)      # the boundary rows are exact zeros (+0.0)
        err = np.abs((got[:, :N].astype(np.clongdouble) - ref))
        ok = bound > 0
        worst['sources conj=%s' % conj] = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
        assert np.all(err[~ok] == 0)
        R2 = torch.zeros_like(R)
        d3.massSourcesDevice(op, dU, k, dW, coef, R2, conj=conj, ldu=ld, ldr=ld)
        assert np.array_equal(bits(R2.cpu().numpy()[:, :N]), bits(got[:, :N]))          # repeated launches: the same bits
    # imaging: accumulation into a non-zero P, the boundary rows of Lambda poisoned
    UF, UB, P0 = s3.randc(rng, (k, ld)), s3.randc(rng, (k, ld)), s3.randc(rng, N)
    UB[:, :N][:, ~inside] = 1e300 * (1 + 1j)
    ref, bound = s3.mass_imaging_reference(dims, UF[:, :N], UB[:, :N], P0)
    dF, dB = _dev(UF), _dev(UB)
    outs = []
    for _ in range(2):
        P = _dev(P0)
        torch.cuda.synchronize()
        d3.massImagingAccumulateDevice(op, dF, dB, k, P, ldf=ld, ldb=ld)
        outs.append(P.cpu().numpy())
    assert np.all(np.isfinite(outs[0].view(np.float64)))      # the mask holds: 1e300 never entered a product
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    err = np.abs(outs[0].astype(np.clongdouble) - ref)
    worst['imaging'] = float((err / bound).max())
    print('%s k=%d: worst error / bound %s' % (dims, k, {n: '%.3f' % v for n, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    del op.factors


def test_chain_kernel_and_refusals(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib, frechet3d
    from zephyr_amd import device_survey3d as d3
    dims = (6, 5, 70)
    op = za.Helm3D(small_config(dims, seed=9))
    N = op.nrow
    rng = np.random.default_rng(2)
    chi = frechet3d.velocityChain3(op)
    dc, P, G0 = rng.standard_normal(N), s3.randc(rng, N), rng.standard_normal(N)
    w = complex(0.4, -0.9)
    W = torch.zeros(N, dtype=torch.complex128, device='cuda:0')
    G = _dev(G0)
    dP, ddc = _dev(P), _dev(dc)
    torch.cuda.synchronize()
    d3.massChainDevice(op, None, w, ddc, W)
    d3.massChainDevice(op, dP, w, None, G)
    # K: c^2, its product with rho and a complex division (about 8 rounded operations); chi: another division (4); w chi and the last product (4): 16
    # operations of relative error u each on either side (numpy's evaluation included), 32 u relative to the magnitudes
    assert np.abs(W.cpu().numpy() - w * chi * dc).max() <= 32 * s3.U53 * np.abs(w * chi * dc).max()
    assert np.abs(G.cpu().numpy() - (G0 + (w * chi * P).real)).max() <= 32 * s3.U53 * (np.abs(G0) + np.abs(w * chi * P)).max()
    # a 2-D handle is refused by all three
    mz = za.MiniZephyr(dict(nx=20, nz=24, dx=10., c=2500., freq=10., nPML=5))
    buf = torch.zeros(4 * 480, dtype=torch.complex128, device='cuda:0')
    p = ctypes.c_void_p(buf.data_ptr())
    assert helm_lib.helm_mass3_sources_device(mz.handle, p, 1, 480, p, 1.0, 0.0, 0, ctypes.c_void_p(buf.data_ptr() + 16 * 960), 480) == -4
    assert '3-D' in _lib.last_error(mz.handle)
    assert helm_lib.helm_mass3_imaging_accumulate_device(mz.handle, p, 480, p, 480, 1, ctypes.c_void_p(buf.data_ptr() + 16 * 960)) == -4
    assert helm_lib.helm_mass3_chain_device(mz.handle, p, 1.0, 0.0, None, p) == -4
    # overlapping or short arguments on a 3-D handle
    big = torch.zeros(4 * N, dtype=torch.complex128, device='cuda:0')
    b = big.data_ptr()
    assert helm_lib.helm_mass3_sources_device(op.handle, ctypes.c_void_p(b), 1, N, ctypes.c_void_p(b + 16 * N), 1.0, 0.0, 0, ctypes.c_void_p(b), N) == -1
    assert helm_lib.helm_mass3_sources_device(op.handle, ctypes.c_void_p(b), 1, N - 1, ctypes.c_void_p(b + 16 * N), 1.0, 0.0, 0, ctypes.c_void_p(b + 32 * N), N) == -1
    assert helm_lib.helm_mass3_imaging_accumulate_device(op.handle, ctypes.c_void_p(b), N, ctypes.c_void_p(b + 16 * N), N, 1, ctypes.c_void_p(b + 16 * N)) == -1
    del op.factors, mz.factors


# ---- 4. the routes ------------------------------------------------------------------------------------------------------------------------------------
ROUTE_DIMS, ROUTE_FREQS = (30, 26, 28), (3., 4.)
_ROUTES = {}


def route_config(mode):
    sc = s3.survey_config(ROUTE_DIMS, 6, ROUTE_FREQS, mode, spacing=(10., 10., 10.), rec_patch=(3, 4), seed=3)
    sc.update(Disc=None, rtol=1e-9, maxit=20000, method='auto', scaleTerm=0.7 - 0.2j)
    del sc['Disc']
    return sc


def device_pair(mode, **extra):
    import zephyr_amd as za
    sc = dict(route_config(mode), **extra)
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def routes(mode):
    'one device pair per receiver mode for the module, with its stored fields and inputs'
    if mode not in _ROUTES:
        prob, sv = device_pair(mode)
        rng = np.random.default_rng(11)
        _ROUTES[mode] = dict(prob=prob, sv=sv, F=prob.fieldsDevice(), r=s3.randc(rng, sv.nD), v=rng.standard_normal(prob.nrow))
    return _ROUTES[mode]


class OracleOnLU(s3.OracleHelm3D):
    'the stand-in with the module\'s shared factors: A^-T from the LU of A'

    def __mul__(self, rhs):
        if sp.issparse(rhs):
            rhs = rhs.toarray()
        lu = lu_of(('route', complex(self.freq)), lambda: s3.oracle_matrix(self))
        x = lu.solve(complex(self.premul) * np.asarray(rhs, dtype=np.complex128), trans='T' if self.transposed else 'N')
        return np.conj(x)


class OracleOnLUT(OracleOnLU, s3.OracleHelm3DT):
    'A^-T from the same factors'


OracleOnLU.Transposed = OracleOnLUT


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_maps_on_the_same_fields(helm_lib, monkeypatch, mode):
    """the kernel routes in isolation: device Jtvec / JvecBorn fed the stored F against the host maps fed the DOWNLOADED F and the downloaded
    back-propagated fields (caught where the device route hands them to the imaging kernel), and what u=None and repeated calls give"""
    import zephyr_amd as za
    from zephyr_amd import _lib, frechet3d
    from zephyr_amd import device_survey3d as d3
    R_ = routes(mode)
    prob, sv, F, r, v = (R_[k] for k in ('prob', 'sv', 'F', 'r', 'v'))
    assert prob._deviceGradientAvailable()
    st = complex(prob.system.scaleTerm)
    Fh = [F[i] for i in range(sv.nfreq)]
    # dpred from the store
    d = sv.dpred(None, u=F).reshape((sv.nrec, sv.nsrc, sv.nfreq))
    for i in range(sv.nfreq):
        for s in range(sv.nsrc):
            assert s3.rel(d[:, s, i], sv.rVec(s, i) @ Fh[i][:, s]) <= 1e-14
    # Jtvec: catch U on its way into the imaging kernel
    caught = []
    real_imaging = d3.massImagingAccumulateDevice

    def imaging(op, d_uf, d_ub, nsrc, d_p, **kw):
        caught.append((complex(op.freq), np.array(_lib.from_device(d_ub).reshape((nsrc, -1)).T)))
        return real_imaging(op, d_uf, d_ub, nsrc, d_p, **kw)
    monkeypatch.setattr(d3, 'massImagingAccumulateDevice', imaging)
    g = prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='operator')
    monkeypatch.setattr(d3, 'massImagingAccumulateDevice', real_imaging)
    assert g.dtype == np.float64 and len(caught) == sv.nfreq
    want = np.zeros(prob.nrow)
    M = frechet3d.massStencil3(ROUTE_DIMS)
    for i, (f, UB) in enumerate(caught):
        op = prob.system.subProblems[i]
        assert f == complex(op.freq)
        Pm = frechet3d.imagingSum3(op, np.conj(Fh[i] / st), np.conj(UB), M)
        want += ((-np.conj(st) / complex(op.premul)) * frechet3d.velocityChain3(op) * Pm).real
    e_g = s3.rel(g, want)
    # JvecBorn: catch the Born sources and the solved columns
    born = []
    real_sources = d3.massSourcesDevice

    def sources(op, d_u, nsrc, d_w, coef, d_r, **kw):
        out = real_sources(op, d_u, nsrc, d_w, coef, d_r, **kw)
        born.append(np.array(_lib.from_device(d_r).reshape((nsrc, -1)).T))
        return out
    monkeypatch.setattr(d3, 'massSourcesDevice', sources)
    J = prob.JvecBorn(None, v, u=F, linearisation='operator')
    monkeypatch.setattr(d3, 'massSourcesDevice', real_sources)
    e_q = max(s3.rel(born[i], frechet3d.bornSources3(prob.system.subProblems[i], v, np.conj(Fh[i] / st), M) / -complex(prob.system.subProblems[i].premul))
              for i in range(sv.nfreq))
    print('%s: device gradient against the host maps on the same fields %.2e, Born sources %.2e' % (mode, e_g, e_q))
    assert e_g <= 1e-12 and e_q <= 1e-12
    # 'full' is 'operator', and repeated calls give the same bits
    assert np.array_equal(bits(prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='full')), bits(g))
    assert np.array_equal(bits(prob.JvecBorn(None, v, u=F, linearisation='full')), bits(J))
    assert np.array_equal(bits(prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='operator')), bits(g))
    assert np.array_equal(bits(prob.JvecBorn(None, v, u=F, linearisation='operator')), bits(J))
    # the adjoint identity on the device: two fields of 1e-6 each multiplied together, and the second solve's amplification
    lhs, rhs = s3.inner(r, J), float(g @ v)
    print('%s: adjoint identity on the device misses by %.2e' % (mode, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    # the reference's gradient: sum_f gradientScaler (.) sum_s uF (.) uB in numpy from downloaded fields -- uB caught on its way into the imaging kernel
    from zephyr_amd import device_survey
    bufs, back = {}, []
    real_buffer, real_img = device_survey.Workspace.buffer, za.Helm3D.imagingAccumulateDevice

    def buffer(self, name, shape):
        bufs[name] = real_buffer(self, name, shape)
        return bufs[name]

    def img(self, d_uf, d_ub, nsrc, d_scaler, d_g, d_exp=None):
        assert bufs['U'].data_ptr() == d_ub
        back.append(np.array(_lib.from_device(bufs['U']).reshape((nsrc, -1)).T))
        return real_img(self, d_uf, d_ub, nsrc, d_scaler, d_g, d_exp=d_exp)
    monkeypatch.setattr(device_survey.Workspace, 'buffer', buffer)
    monkeypatch.setattr(za.Helm3D, 'imagingAccumulateDevice', img)
    g0 = prob.Jtvec(None, r, u=F)
    monkeypatch.setattr(device_survey.Workspace, 'buffer', real_buffer)
    monkeypatch.setattr(za.Helm3D, 'imagingAccumulateDevice', real_img)
    assert g0.dtype == np.float64 and len(back) == sv.nfreq
    want0 = sum(np.asarray(prob.gradientScaler(i)).ravel() * (Fh[i] * (st * back[i])).sum(axis=1) for i in range(sv.nfreq)).real
    print('%s: default Jtvec against numpy on downloaded fields %.2e' % (mode, s3.rel(g0, want0)))
    assert s3.rel(g0, want0) <= 1e-12


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_end_to_end_against_the_sparse_lu(helm_lib, mode):
    "gradient and Born data at rtol = 1e-9 against the host route on splu: 1e-5 allows two fields of 1e-6 each multiplied together and the second solve"
    import zephyr_amd as za
    R_ = routes(mode)
    prob, sv, F, r, v = (R_[k] for k in ('prob', 'sv', 'F', 'r', 'v'))
    sc = dict(route_config(mode), Disc=OracleOnLU, hostGradient=True)
    hp, hs = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    hp.pair(hs)
    g, J = prob.Jtvec(None, r, u=F, adjoint='transpose', linearisation='operator'), prob.JvecBorn(None, v, u=F, linearisation='operator')
    gh, Jh = hp.Jtvec(None, r, adjoint='transpose', linearisation='operator'), hp.JvecBorn(None, v, linearisation='operator')
    e = dict(gradient=s3.rel(g, gh), born=s3.rel(J, Jh), dpred=s3.rel(sv.dpred(None, u=F), hs.dpred(None)))
    print('%s: device routes against the host route on splu %s' % (mode, {k: '%.2e' % x for k, x in e.items()}))
    assert e['gradient'] <= 1e-5 and e['born'] <= 1e-5 and e['dpred'] <= 1e-6


def test_taylor_remainders_through_the_device_routes(helm_lib):
    R_ = routes('fixed')
    prob, sv, F = R_['prob'], R_['sv'], R_['F']
    c0 = np.array(prob.systemConfig['c'])
    rng = np.random.default_rng(21)
    dc = 120. * rng.uniform(-1., 1., c0.shape)
    d0 = sv.dpred(None, u=F)
    J = prob.JvecBorn(None, dc.ravel(), u=F, linearisation='operator')
    p2, s2 = device_pair('fixed')
    rem = [np.linalg.norm(s2.dpred(c0 + 0.5 ** j * dc) - d0 - 0.5 ** j * J) for j in range(4)]
    ratios = [rem[j] / rem[j + 1] for j in range(3)]
    print('Taylor remainders through the device routes %s, ratios %s, rtol |d| = %.1e' % (['%.3e' % x for x in rem], ['%.3f' % x for x in ratios], 1e-9 * np.linalg.norm(d0)))
    assert rem[-1] >= 100 * 1e-9 * np.linalg.norm(d0)          # the smallest remainder stays 100 x above the solver's tolerance
    assert all(3.8 <= x <= 4.2 for x in ratios), ratios
    del p2.factors


def test_scaler_illumination_and_released_factors(helm_lib):
    R_ = routes('fixed')
    prob, sv, F = R_['prob'], R_['sv'], R_['F']
    Fh = [F[i] for i in range(sv.nfreq)]
    H = prob.illumination(None, u=F, kind='energy')
    assert s3.rel(H, sum((np.abs(f) ** 2).sum(axis=1) for f in Fh)) <= 1e-13
    assert prob.adjointSystem is not prob.system and all(s.transposed for s in prob.adjointSystem.subProblems)
    del prob.factors
    assert not prob.factors and not prob.adjointSystem.factors


RANKS = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
os.environ['HELM_DEVICES'] = '0'
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import survey3d_cases as s3
from tests.test_gpu_survey3d import device_pair
ref, sref = device_pair('relative', shardFreqs=False)
prob, sv = device_pair('relative')
assert prob._deviceGradientAvailable() and prob.ownedFreqs == [dist.get_rank()] and ref.ownedFreqs == [0, 1]
rng = np.random.default_rng(11)
r, v = s3.randc(rng, sv.nD), rng.standard_normal(prob.nrow)
F = prob.fieldsDevice()
assert F.ownedFreqs == prob.ownedFreqs
T = dict(adjoint='transpose', linearisation='operator')
# the gradient to 1e-12 (its solves have the same history on both sides and come out the same to the bit); the other three re-solve on handles that have
# solved before, and two solves of one system at rtol = 1e-9 agree to the suite's 3-D tolerance at this rtol, 1e-6
e = [s3.rel(prob.Jtvec(None, r, u=F, **T), ref.Jtvec(None, r, **T)), s3.rel(prob.JvecBorn(None, v, u=F, linearisation='operator'), ref.JvecBorn(None, v, linearisation='operator')),
     s3.rel(sv.dpred(None, u=F), sref.dpred(None)), s3.rel(prob.Jtvec(None, r, u=F), ref.Jtvec(None, r, u=ref.fields()))]
print('RANK', dist.get_rank(), ['%%.2e' %% x for x in e], flush=True)
ok = e[0] <= 1e-12 and max(e[1:]) <= 1e-6
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_gradient(helm_lib, tmp_path):
    "the two frequencies sharded over two ranks on one GPU: the all-reduce of the (N,) vector (of the data for JvecBorn) gives every rank the single-rank result"
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'ranks.py'
    script.write_text(RANKS % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29671', WORLD_SIZE='2', PYTHONPATH=root)
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


def test_u_none_is_bit_identical_to_the_stored_fields(helm_lib):
    """u=None solves the forward fields into HBM, runs the route of u=F and releases them: the same bits as fieldsDevice() followed by u=F.  Compared on
    fresh pairs, so that every solve has the same history on both sides: a handle of the 3-D Krylov path that has solved before does not repeat a solve to
    the bit (measured on the MI355X: dpred from a second solve differs from the stored fields' by 1e-9 .. 4e-9 at rtol = 1e-9, the first entries of a
    gradient -- corner nodes, where both fields have decayed below the tolerance -- entirely), which is the solver's and not the route's."""
    rng = np.random.default_rng(11)
    T = dict(adjoint='transpose', linearisation='operator')
    out = []
    for stored in (False, True):
        pg, sg = device_pair('relative')
        pb, sb = device_pair('relative')
        r, v = s3.randc(rng, sg.nD) if not out else out[0][2], rng.standard_normal(pg.nrow) if not out else out[0][3]
        Fg, Fb = (pg.fieldsDevice(), pb.fieldsDevice()) if stored else (None, None)
        out.append((pg.Jtvec(None, r, u=Fg, **T), pb.JvecBorn(None, v, u=Fb, linearisation='operator'), r, v))
        del pg.factors, pb.factors
    print('u=None against u=F on fresh pairs: gradient %.2e, Born data %.2e' % (s3.rel(out[0][0], out[1][0]), s3.rel(out[0][1], out[1][1])))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
