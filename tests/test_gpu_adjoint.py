"""GPU: the transposed MiniZephyr operator (helm_set_transposed) and what stands on it -- the planes against the numpy formula bit for bit, the transposed
solve against SuperLU on the direct and the Krylov paths, the condition estimate of the direct solver on a transposed handle, the virtual-source kernel
against an extended-precision evaluation, and Jtvec(adjoint='transpose') / JvecBorn / Hvec end to end on a rough model against the host route on the
oracle doubles, with solves and transfers counted."""
import ctypes
import hashlib
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
U_RND = 2.0 ** -53
rel, randc, inner = ac.rel, ac.randc, ac.inner


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. transposed planes ------------------------------------------------------------------------------------------------------------------
PLANE_CASES = {
    '37x53-freesurf': dict(nz=37, nx=53, dx=10., dz=10., nPML=6, freeSurf=(True, False, False, False)),
    '64x64-ky': dict(nz=64, nx=64, dx=10., dz=10., nPML=8, ky=0.003),
    '5x300-dx-ne-dz': dict(nz=5, nx=300, dx=10., dz=7., nPML=4),
}


@pytest.mark.parametrize('case', sorted(PLANE_CASES))
def test_transposed_planes_are_the_numpy_formula_bit_for_bit_and_toggle_back(helm_lib, case):
    import zephyr_amd as za
    from zephyr_amd import _lib
    kw = PLANE_CASES[case]
    cfg = dict(kw, c=ac.rough_model(kw['nz'], kw['nx'], 4), freq=20.)
    plain, tr = za.MiniZephyr(cfg), za.MiniZephyr(dict(cfg, transposed=True))
    C, CT = plain.diagonals()[0], tr.diagonals()[0]
    assert helm_lib.helm_get_transposed(plain.handle) == 0 and helm_lib.helm_get_transposed(tr.handle) == 1
    assert np.array_equal(bits(CT), bits(ac.transpose_planes(C)))
    assert not np.array_equal(bits(CT), bits(C))
    # the flag off and a re-assembly: the plain planes again; on again: the transposed ones
    h = tr.handle
    f = complex(tr.freq)
    for on, want in ((0, C), (1, CT)):
        _lib.check(helm_lib.helm_set_transposed(h, on), h)
        assert helm_lib.helm_get_transposed(h) == 1 - on          # in force from the next assembly only
        _lib.check(helm_lib.helm_assemble(h, f.real, f.imag, float(tr.tau), float(tr.ky), 0.0), h)
        assert helm_lib.helm_get_transposed(h) == on
        assert np.array_equal(bits(tr.diagonals()[0]), bits(want))
    del plain.factors, tr.factors


def test_eurus_and_3d_handles_refuse_the_flag(helm_lib):
    import zephyr_amd as za
    from zephyr_amd import _lib
    eu = za.Eurus(dict(nx=40, nz=36, dx=10., c=2500., freq=10., nPML=6))
    assert helm_lib.helm_set_transposed(eu.handle, 1) == -4              # HELM_ERR_UNSUPPORTED
    assert 'MiniZephyr' in _lib.last_error(eu.handle)
    assert helm_lib.helm_get_transposed(eu.handle) == 0
    h3 = za.Helm3D(dict(nx=16, ny=12, nz=14, dx=10., c=2500., rho=1., freq=10., nPML=4, cPML=200.))
    assert helm_lib.helm_set_transposed(h3.handle, 1) == -4
    assert helm_lib.helm_set_transposed(None, 1) == -1
    del eu.factors, h3.factors


# ---- 2. the transposed solve against SuperLU ------------------------------------------------------------------------------------------------
def superlu_transposed(op, q):
    'conj(A^-T (premul q)) from the oracle matrix of the PLAIN operator and splu(...).solve(..., trans=\'T\')'
    C = ho.minizephyr_coefficients(int(op.nz), int(op.nx), op.c, ho.gardner_rho(op.c), complex(op.freq), dx=op.dx, dz=op.dz, nPML=int(op.nPML), ky=op.ky,
                                   freeSurf=op.freeSurf)
    lu = spla.splu(ho.coefficients_to_csr(C).tocsc())
    return np.conj(lu.solve(complex(op.premul) * np.asarray(q, dtype=np.complex128), trans='T'))


def tree_depth(lib, nz, nx):
    from zephyr_amd import _lib
    leaf = int(_lib.tuning().nd_leaf)
    n = lib.helm_direct_plan(nz, nx, leaf, None, 0)
    plan = np.zeros((n, 12), dtype=np.int32)
    assert lib.helm_direct_plan(nz, nx, leaf, plan.ctypes.data_as(P), n) == n

    def depth(i):
        kids = [k for k in (plan[i, 8], plan[i, 9]) if k >= 0]
        return 1 + max(depth(k) for k in kids) if kids else 0
    return n, depth(n - 1)


SOLVE_CASES = {
    #                 class           grid      nPML  method      free surface
    'leaf-direct':   ('MiniZephyr',   (8, 8),   3,    'direct',   (False, False, False, False)),
    'tree-direct':   ('MiniZephyrHD', (37, 53), 6,    'direct',   (True, False, False, False)),
    'bicgstab':      ('MiniZephyr',   (40, 50), 8,    'bicgstab', (False, False, False, False)),
    'mg':            ('MiniZephyr',   (70, 90), 8,    'mg',       (False, False, False, False)),
}


@pytest.mark.parametrize('case', sorted(SOLVE_CASES))
def test_transposed_solve_matches_superlu_and_differs_from_the_plain_one(helm_lib, case):
    import zephyr_amd as za
    cls, (nz, nx), npml, method, fs = SOLVE_CASES[case]
    if case == 'leaf-direct':
        assert tree_depth(helm_lib, nz, nx) == (1, 0)                   # one front: the leaf
    if case == 'tree-direct':
        assert tree_depth(helm_lib, nz, nx)[1] >= 3                     # at least three separator levels above the leaves
    freq = 9. if method == 'mg' else 20.
    cfg = dict(nx=nx, nz=nz, dx=10., dz=8., c=ac.rough_model(nz, nx, 6), freq=freq, nPML=npml, freeSurf=fs, rtol=1e-10, method=method, maxit=400000)
    rng = np.random.default_rng(2)
    X, Z = 10. * (nx - 1), 8. * (nz - 1)
    locs = np.stack([rng.uniform(0.3 * X, 0.7 * X, 3), rng.uniform(0.3 * Z, 0.7 * Z, 3)], axis=1)
    q_sparse = za.SparseKaiserSource(cfg)(locs) if min(nz, nx) >= 20 else za.SimpleSource(cfg)(locs)
    q_dense = randc(rng, (nz * nx, 5))
    tr, plain = getattr(za, cls)(dict(cfg, transposed=True)), getattr(za, cls)(cfg)
    for q in (q_sparse, q_dense):
        qd = q.toarray() if hasattr(q, 'toarray') else np.asarray(q)
        u = tr * q
        info = tr.lastInfo
        ref = superlu_transposed(tr, qd)
        err = rel(u, ref)
        print('%s: transposed solve against SuperLU rel-L2 %.2e, worst relres %.2e' % (case, err, max(i['relres'] for i in info)))
        assert err <= 1e-7, info
        assert all(i['relres'] <= 1e-10 for i in info), info
        assert rel(plain * q, u) > 1e-3                                 # (a model on which A^-T and A^-1 differ: otherwise this shows nothing)
    del tr.factors, plain.factors


# ---- 3. NdStable on a transposed handle -----------------------------------------------------------------------------------------------------
def test_no_front_of_a_well_conditioned_transposed_operator_is_treated_and_factors_are_reproducible(helm_lib, monkeypatch, capfd):
    """The model of test_gpu_stable_fronts' case (a), transposed.  The identity rows of A are columns e_j of A^T: the estimate is formed of the transposed
    front there, so no front is handed to the pivoted LU, and eight factorisations give the same bits."""
    import torch
    import zephyr_amd as za
    nz, nx, nrhs = 150, 170, 9
    rng = np.random.default_rng(11)
    c = 2500. + 500. * np.sin(np.arange(nz)[:, None] / 20.) * np.ones((nz, nx))
    cfg = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, freq=8., nPML=8, rtol=1e-10, method='direct', batch=256, transposed=True)
    locs = np.stack([rng.uniform(100., 10. * nx - 100., nrhs), rng.uniform(20., 60., nrhs)], axis=1)
    q = np.ascontiguousarray(za.SparseKaiserSource(cfg)(locs).toarray())

    def solve():
        op = za.MiniZephyr(cfg)
        R = torch.from_numpy(q).cuda()
        U = torch.empty_like(R)
        op.solveDevice(R.data_ptr(), U.data_ptr(), nrhs, nz * nx, layout='node')
        torch.cuda.synchronize()
        info = [dict(i) for i in op.lastInfo]
        del op.factors
        return U.cpu().numpy(), info

    monkeypatch.setenv('HELM_ND_DEBUG', '1')
    seen = set()
    for k in range(8):
        u, info = solve()
        seen.add(hashlib.sha1(u.tobytes()).hexdigest())
        assert all(i['iterations'] == 1 and i['relres'] <= 1e-10 for i in info), info
    err = capfd.readouterr().err
    treated = sum(int(m) for m in re.findall(r'(\d+) ill-conditioned front\(s\) re-eliminated', err))
    assert treated == 0, 'fronts of a well-conditioned transposed MiniZephyr operator handed to the pivoted LU: %d' % treated
    assert len(seen) == 1, 'factorisations of one transposed operator gave %d different wavefield arrays' % len(seen)


# ---- 4. the virtual-source kernel ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def op4800(helm_lib):
    import zephyr_amd as za
    o = za.MiniZephyr(dict(nx=80, nz=60, dx=10., dz=10., c=2500., freq=5., nPML=6))
    assert o.nrow == 4800 and o.nrow % 256 != 0 and o.handle
    yield o
    del o.factors


@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('nsrc', [1, 8, 13])
def test_virtual_sources_kernel_against_extended_precision(helm_lib, op4800, nsrc, fmt):
    """R[s ldr + i] = conj(W[i] u[s ldu + i]) against a longdouble evaluation, per component within 3 * 2^-53 (|Re W||Re u| + |Im W||Im u|) for the real part
    and 3 * 2^-53 (|Re W||Im u| + |Im W||Re u|) for the imaginary part (two rounded products and one rounded sum, contracted or not; the conjugation is
    exact); u is the exactly unpacked value for the complex64 store.  ldu, ldr > N; the guard cells around R and the gaps between its columns stay as
    they were; two runs give the same bits."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference, unpack_reference
    op = op4800
    dev = torch.device('cuda', op.device)
    N, ldu, ldr, guard = op.nrow, op.nrow + 38, op.nrow + 11, 1031
    rng = np.random.default_rng(70 + nsrc)
    U = randc(rng, (N, nsrc)) * 10.0 ** rng.uniform(-8, 8, nsrc)[None, :] * 10.0 ** rng.uniform(-6, 0, (N, nsrc))
    W = randc(rng, N) * 10.0 ** rng.uniform(-4, 4, N)
    Upad = np.zeros((nsrc, ldu), dtype=np.complex128)
    dW = torch.from_numpy(W).to(dev)
    if fmt == 'complex64':
        Pk, e = pack_reference(U)
        Uh = unpack_reference(Pk, e)
        Ppad = np.zeros((nsrc, ldu), dtype=np.complex64)
        Ppad[:, :N] = Pk.T
        dU, dE = torch.from_numpy(Ppad).to(dev), torch.from_numpy(e).to(dev)
    else:
        Uh = U
        Upad[:, :N] = U.T
        dU = torch.from_numpy(Upad).to(dev)
    fill = complex(7.0, -3.0)
    runs = []
    for _ in range(2):
        out = torch.full((2 * guard + nsrc * ldr,), fill, dtype=torch.complex128, device=dev)
        torch.cuda.synchronize(dev)
        if fmt == 'complex64':
            _lib.check(helm_lib.helm_virtual_sources_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), nsrc, ldu, P(dW.data_ptr()), P(out.data_ptr() + 16 * guard), ldr), op.handle)
        else:
            _lib.check(helm_lib.helm_virtual_sources_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dW.data_ptr()), P(out.data_ptr() + 16 * guard), ldr), op.handle)
        h = out.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + nsrc * ldr:] == fill)
        body = h[guard:guard + nsrc * ldr].reshape((nsrc, ldr))
        assert np.all(body[:, N:] == fill)                              # the gap between two columns of R
        runs.append(body[:, :N].T.copy())
    R = runs[0]
    assert np.array_equal(bits(R), bits(runs[1]))
    ld = np.longdouble
    wr, wi, ur, ui = W.real.astype(ld)[:, None], W.imag.astype(ld)[:, None], Uh.real.astype(ld), Uh.imag.astype(ld)
    ref_re, ref_im = wr * ur - wi * ui, -(wr * ui + wi * ur)
    b_re = 3 * U_RND * (np.abs(wr) * np.abs(ur) + np.abs(wi) * np.abs(ui))
    b_im = 3 * U_RND * (np.abs(wr) * np.abs(ui) + np.abs(wi) * np.abs(ur))
    e_re, e_im = np.abs(R.real.astype(ld) - ref_re), np.abs(R.imag.astype(ld) - ref_im)
    worst = max(float((e_re[b_re > 0] / b_re[b_re > 0]).max()), float((e_im[b_im > 0] / b_im[b_im > 0]).max()))
    print('virtual_sources %s nsrc=%d: worst err / bound = %.3f' % (fmt, nsrc, worst))
    assert (e_re <= b_re).all() and (e_im <= b_im).all(), worst
    # bad arguments are refused before anything is launched
    assert helm_lib.helm_virtual_sources_device(op.handle, P(dU.data_ptr()), nsrc, N - 1, P(dW.data_ptr()), P(out.data_ptr()), ldr) == -1
    assert helm_lib.helm_virtual_sources_device(op.handle, P(dU.data_ptr()), 0, ldu, P(dW.data_ptr()), P(out.data_ptr()), ldr) == -1
    assert helm_lib.helm_virtual_sources_device(op.handle, P(dU.data_ptr()), nsrc, ldu, P(dW.data_ptr()), P(out.data_ptr() + 8), ldr) == -1
    if fmt == 'complex64':          # no field, no exponents, values off 8 bytes, exponents off 4, ld < N, the output on the field
        u, e, r = dU.data_ptr(), dE.data_ptr(), P(out.data_ptr())
        for pu, pe, l, pr in ((None, P(e), ldu, r), (P(u), None, ldu, r), (P(u + 4), P(e), ldu, r), (P(u), P(e + 2), ldu, r), (P(u), P(e), N - 1, r), (P(u), P(e), ldu, P(u))):
            assert helm_lib.helm_virtual_sources_c64_device(op.handle, pu, pe, nsrc, l, P(dW.data_ptr()), pr, ldr) == -1


# ---- 5. end to end on the device -----------------------------------------------------------------------------------------------------------
NZ, NX, NSRC, NREC = 96, 80, 13, 7
FREQS = (12., 16., 20.)
E2E = {'fixed': ('MiniZephyr', 'OracleMiniZephyrT', dict(freeSurf=(True, False, False, False))),
       'relative': ('MiniZephyrHD', 'OracleMiniZephyrHDT', dict(scaleTerm=0.7 - 0.2j))}


def device_pair(mode, **extra):
    import zephyr_amd as za
    sc = ac.survey_config(NZ, NX, NSRC, NREC, FREQS, mode, nPML=8)
    del sc['parallel']
    sc.update(Disc=getattr(za, E2E[mode][0]), rtol=1e-11, **E2E[mode][2])
    sc.update(extra)
    prob, sv = ac.Helm2DProblem(sc), ac.Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def host_pair(mode, **extra):
    sc = ac.survey_config(NZ, NX, NSRC, NREC, FREQS, mode, nPML=8)
    sc.update(Disc=getattr(ac, E2E[mode][1]), hostGradient=True, **E2E[mode][2])
    sc.update(extra)
    prob, sv = ac.Helm2DProblem(sc), ac.Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


@pytest.fixture(scope='module')
def host_ref():
    'per mode, from the oracle doubles on the host route, made once: fields, a model vector, a residual, JvecBorn v, the transposed gradient and its magnitude sum'
    out = {}
    for mode in ('fixed', 'relative'):
        probh, svh = host_pair(mode)
        rng = np.random.default_rng(31)
        v, r = rng.standard_normal(probh.nrow), randc(rng, svh.nD)
        uF = probh.fields()
        qb = svh.getResidualSources(r.reshape((svh.nrec, svh.nsrc, svh.nfreq)))
        M = np.zeros(probh.nrow)
        for ifreq, uB in probh._solveOwned(qb, probh.adjointSystem):
            M += np.abs(probh.gradientScaler(ifreq)) * (np.abs(uF[ifreq]) * np.abs(uB)).sum(axis=1)
        out[mode] = dict(prob=probh, sv=svh, v=v, r=r, uF=uF, M=M, Jv=probh.JvecBorn(None, v, u=uF), gT=probh.Jtvec(None, r, u=uF, adjoint='transpose'))
    return out


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_complex128_store_against_the_host_route_identity_hvec_and_u_none(helm_lib, monkeypatch, host_ref, mode):
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, r = h['v'], h['r']
    prob, sv = device_pair(mode)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    gT = prob.Jtvec(None, r, u=F, adjoint='transpose')
    Jv = prob.JvecBorn(None, v, u=F)
    assert gT.shape == (prob.nrow,) and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128
    eg, ej = rel(gT, h['gT']), rel(Jv, h['Jv'])
    lhs = inner(Jv, r)
    miss = abs(lhs - inner(v, gT)) / abs(lhs)
    miss_default = abs(lhs - inner(v, prob.Jtvec(None, r, u=F))) / abs(lhs)
    print('%s complex128: Jtvec(transpose) against the host route %.2e, JvecBorn %.2e; identity misses by %.2e (default Jtvec: %.2e)' % (mode, eg, ej, miss, miss_default))
    assert eg <= 1e-6 and ej <= 1e-6
    assert miss <= 1e-7
    assert miss_default > 1e-2
    # u = None: fieldsDevice inside, the same launches on the same inputs
    assert np.array_equal(bits(prob.Jtvec(None, r, adjoint='transpose')), bits(gT))
    assert np.array_equal(bits(prob.JvecBorn(None, v)), bits(Jv))
    # Hvec: symmetric on two random pairs, positive, and equal to its halves
    rng = np.random.default_rng(37)
    for _ in range(2):
        x, y = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow)
        Hx, Hy = prob.Hvec(None, x, u=F), prob.Hvec(None, y, u=F)
        a, b = float(x @ Hy), float(Hx @ y)
        assert abs(a - b) <= 1e-7 * max(abs(a), abs(b)), (a, b)
        assert float(x @ Hx) > 0
    assert np.array_equal(bits(prob.Hvec(None, v, u=F)), bits(prob.Jtvec(None, prob.JvecBorn(None, v, u=F), u=F, adjoint='transpose')))
    assert rel(prob.Hvec(None, v), prob.Hvec(None, v, u=F)) <= 1e-12
    F.release()
    with pytest.raises(ValueError):
        prob.JvecBorn(None, v, u=F)
    F2 = prob.fieldsDevice()
    prob.updateModel(prob.systemConfig['c'] * 1.01)
    with pytest.raises(ValueError):
        prob.Jtvec(None, r, u=F2, adjoint='transpose')
    with pytest.raises(ValueError):
        prob.Hvec(None, v, u=F2)
    F2.release()
    del prob.factors


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_complex64_store_within_the_format_bound(helm_lib, monkeypatch, host_ref, mode):
    """Every stored component is within 2^-24 relative of the solved one.  Gradient: |g64 - g128| <= 2 * 2^-24 * M per point, M = sum_f |w_f| sum_s |uF_s||uB_s|
    from host solves (the bound of test_gpu_fieldstore).  Born data: the virtual sources inherit the 2^-24, so per datum
    |d64 - d128| <= 2 * 2^-24 |scaleTerm| |R| |A^-1| |premul| (|v w_f| (.) |uF_s|) with the entrywise |A^-1| (its rows at the receiver cells, from the oracle;
    fixed array, whose receivers touch few cells).  Both modes: JvecBorn on the packed store against the host route on the UNPACKED fields to 1e-6, and the
    adjoint identity, whose two sides read the same store."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    h = host_ref[mode]
    v, r, probh, svh = h['v'], h['r'], h['prob'], h['sv']
    prob, sv = device_pair(mode)
    prob64, sv64 = device_pair(mode, fieldsDtype='complex64')
    F, F64 = prob.fieldsDevice(), prob64.fieldsDevice()
    assert F64.dtype == 'complex64' and 2 * sum(F64.nbytes.values()) < 1.01 * sum(F.nbytes.values())
    g128, g64 = prob.Jtvec(None, r, u=F, adjoint='transpose'), prob64.Jtvec(None, r, u=F64, adjoint='transpose')
    d128, d64 = prob.JvecBorn(None, v, u=F), prob64.JvecBorn(None, v, u=F64)
    err = np.abs(g64 - g128)
    M = h['M']
    print('%s complex64: worst |g64 - g128| / (2 * 2^-24 M) = %.3f; rel = %.2e' % (mode, float((err[M > 0] / (2 * 2.0 ** -24 * M[M > 0])).max()), rel(g64, g128)))
    assert (err <= 2 * 2.0 ** -24 * M).all()
    assert rel(g64, g128) > 0 and rel(d64, d128) > 0                   # (the packed store was read)
    if mode == 'fixed':
        shape = (sv.nrec, sv.nsrc, sv.nfreq)
        bound = np.zeros(shape)
        sigma = abs(complex(probh.system.scaleTerm))
        for f in range(sv.nfreq):
            Rm = abs(svh.rVec(0, f)).tocsc()
            cells = np.flatnonzero(np.diff(Rm.indptr))
            cols = np.zeros((probh.nrow, cells.size))
            cols[cells, np.arange(cells.size)] = 1.0
            E = np.abs(probh.adjointSystem.subProblems[f] * cols).T                   # |premul| |A^-1|[cells, :]
            T = np.abs(v * np.asarray(probh.gradientScaler(f)).ravel())[:, None] * np.abs(h['uF'][f])
            bound[:, :, f] = 2 * 2.0 ** -24 * sigma * np.asarray(Rm[:, cells] @ (E @ T))
        derr = np.abs(d64 - d128).reshape(shape)
        print('%s complex64: worst |d64 - d128| / bound = %.3f; rel = %.2e' % (mode, float((derr / bound).max()), rel(d64, d128)))
        assert (derr <= bound).all()
    dh = probh.JvecBorn(None, v, u=list(F64))                            # the host route on what the packed store unpacks to
    assert rel(d64, dh) <= 1e-6
    lhs = inner(d64, r)
    assert abs(lhs - inner(v, g64)) <= 1e-7 * abs(lhs)
    F.release(), F64.release()
    del prob.factors, prob64.factors


def test_25d_composite_keeps_the_identity(helm_lib, monkeypatch):
    'nky = 2, the ky sum formed in HBM: both solves of every ky are transposed together, and the identity holds on the sums'
    import zephyr_amd as za
    monkeypatch.setenv('HELM_DEVICES', '0')
    sc = ac.survey_config(NZ, NX, NSRC, NREC, FREQS, 'fixed', nPML=8)
    sc.update(Disc=za.MiniZephyr25D, nky=2, rtol=1e-11)
    prob, sv = ac.Helm25DProblem(sc), ac.Helm25DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    rng = np.random.default_rng(41)
    v, r = rng.standard_normal(prob.nrow), randc(rng, sv.nD)
    F = prob.fieldsDevice()
    Jv, gT = prob.JvecBorn(None, v, u=F), prob.Jtvec(None, r, u=F, adjoint='transpose')
    lhs = inner(Jv, r)
    miss = abs(lhs - inner(v, gT)) / abs(lhs)
    print('2.5-D nky=2: identity misses by %.2e' % miss)
    assert miss <= 1e-7
    assert abs(lhs - inner(v, prob.Jtvec(None, r, u=F))) > 1e-2 * abs(lhs)
    F.release()
    del prob.factors


def test_two_workers_on_one_gpu_agree_with_one(helm_lib, monkeypatch):
    'one frequency, two workers on GPU 0: the store is dealt 0:6 / 6:13 and the transposed wrapper supplies the replica of the second batch'
    one = dict(freqs=[FREQS[1]], sterms=np.array([0.8 - 0.3j]))
    rng = np.random.default_rng(43)
    res = []
    for devs in ('0', '0,0'):
        monkeypatch.setenv('HELM_DEVICES', devs)
        prob, sv = device_pair('relative', **one)
        assert len(prob.system.devices) == len(devs.split(','))
        if not res:
            v, r = rng.standard_normal(prob.nrow), randc(rng, sv.nD)
        F = prob.fieldsDevice()
        assert [(c0, c1) for _, _, _, c0, c1 in F.items] == ([(0, 13)] if devs == '0' else [(0, 6), (6, 13)])
        res.append((prob.Jtvec(None, r, u=F, adjoint='transpose'), prob.JvecBorn(None, v, u=F), prob.Hvec(None, v, u=F)))
        F.release()
        del prob.factors
    for a, b in zip(res[1], res[0]):
        assert rel(a, b) <= 1e-9


def test_counts_columns_solved_and_bytes_moved(helm_lib, monkeypatch):
    """Patched as test_gpu_fieldstore's counting test: JvecBorn(u=F) solves nsrc columns per frequency and brings down nrec * nsrc * 16 bytes per frequency;
    Hvec(u=F) solves 2 nsrc columns per frequency; no host-array solve, and nothing of N x nsrc values crosses PCIe in either direction."""
    from zephyr_amd import _lib
    from zephyr_amd.discretization import BaseDiscretization
    monkeypatch.setenv('HELM_DEVICES', '0')
    counts = dict(solve=0, cols=[], down=[], up=[])
    real_solve, real_sd, real_fd, real_fdp, real_td = BaseDiscretization._solve, BaseDiscretization.solveDevice, _lib.from_device, _lib.from_device_pinned, _lib.to_device

    def solve(self, rhs, rows):
        counts['solve'] += 1
        return real_solve(self, rhs, rows)

    def solve_device(self, d_rhs, d_u, nrhs, *a, **k):
        counts['cols'].append(int(nrhs))
        return real_sd(self, d_rhs, d_u, nrhs, *a, **k)

    def counting(fn):
        def wrapped(t):
            counts['down'].append(t.numel() * t.element_size())
            return fn(t)
        return wrapped

    def to_device(arr, dev, dtype=None):
        counts['up'].append(np.asarray(arr).size * np.dtype(dtype if dtype is not None else np.asarray(arr).dtype).itemsize)
        return real_td(arr, dev, dtype)
    monkeypatch.setattr(BaseDiscretization, '_solve', solve)
    monkeypatch.setattr(BaseDiscretization, 'solveDevice', solve_device)
    monkeypatch.setattr(_lib, 'from_device', counting(real_fd))
    monkeypatch.setattr(_lib, 'from_device_pinned', counting(real_fdp))
    monkeypatch.setattr(_lib, 'to_device', to_device)
    rng = np.random.default_rng(47)
    for mode in ('fixed', 'relative'):
        prob, sv = device_pair(mode)
        N, nfreq, nsrc, nrec = prob.nrow, sv.nfreq, sv.nsrc, sv.nrec
        v, r = rng.standard_normal(N), randc(rng, sv.nD)
        F = prob.fieldsDevice()
        counts.update(solve=0, cols=[], down=[], up=[])
        prob.JvecBorn(None, v, u=F)
        assert (counts['solve'], counts['cols'], sorted(counts['down'])) == (0, [nsrc] * nfreq, [nrec * nsrc * 16] * nfreq)
        assert max(counts['up']) < N * nsrc * 16
        counts.update(cols=[], down=[], up=[])
        prob.Jtvec(None, r, u=F, adjoint='transpose')
        assert (counts['solve'], counts['cols'], counts['down']) == (0, [nsrc] * nfreq, [N * 16])
        counts.update(cols=[], down=[], up=[])
        prob.Hvec(None, v, u=F)
        assert counts['solve'] == 0 and counts['cols'] == [nsrc] * (2 * nfreq)
        assert sorted(counts['down']) == [nrec * nsrc * 16] * nfreq + [N * 16]
        assert max(counts['up']) < N * nsrc * 16
        F.release()
        del prob.factors


# ---- 6. nothing existing moved -------------------------------------------------------------------------------------------------------------
def test_existing_routes_give_the_same_bits_before_and_after_the_transposed_wrapper_is_used(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = device_pair('fixed')
    rng = np.random.default_rng(53)
    v, r = rng.standard_normal(prob.nrow), randc(rng, sv.nD)
    F = prob.fieldsDevice()

    def existing():
        return [prob.Jtvec(None, r), prob.Jtvec(None, r, u=F), sv.dpred(), sv.dpred(u=F), prob.illumination(u=F), prob.illumination()]
    before = existing()
    assert '_adjointSystem' not in prob.__dict__
    prob.Hvec(None, v, u=F)
    prob.Jtvec(None, r, adjoint='transpose')
    assert prob.adjointSystem.factors
    after = existing()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    F.release()
    del prob.factors
    assert not prob.adjointSystem.factors and not prob.system.factors
