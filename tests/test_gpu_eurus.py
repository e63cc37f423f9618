"""GPU: what the config key eurusDerivatives serves on Eurus operators with eps == delta -- M1^T in the handle (helm_set_transposed_m1) bit for bit and its
refusals, the transposed solve against SuperLU, the three derivative kernels through their C entry points against the 80-bit evaluations of
tests/eurus_cases.py under its componentwise bounds, the device routes of Jtvec / JvecBorn / Hvec against the host route fed the downloaded fields (both
stores, two workers, a moving array, the Gardner density), the Taylor test of dpred through the device routes, and that a MiniZephyr problem and an Eurus
problem without the key give the same bits before and after."""
import ctypes

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import helm_oracle as ho
from tests import adjoint_cases as ac
from tests import eurus_cases as ec

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
rel, randc, inner = ac.rel, ac.randc, ac.inner


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. transposed planes and what a transposed handle refuses ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('aniso', ec.ANISO)
def test_block_0_holds_the_transposed_planes_bit_for_bit_and_toggles_back(helm_lib, aniso):
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = ec.operator_config('37x53', aniso)
    plain, tr = za.Eurus(sc), za.Eurus(dict(sc, transposed=True))
    C, CT = plain.diagonals()[0], tr.diagonals()
    assert CT.shape == (1, 9, 37, 53)
    assert helm_lib.helm_get_transposed(plain.handle) == 0 and helm_lib.helm_get_transposed(tr.handle) == 1
    assert np.array_equal(bits(CT[0]), bits(ac.transpose_planes(C)))
    assert not np.array_equal(bits(CT[0]), bits(C))
    h = tr.handle
    f = complex(tr.freq)
    out = np.empty((9, 37, 53), dtype=np.complex128)
    for on, want in ((0, C), (1, CT[0])):
        _lib.check(helm_lib.helm_set_transposed_m1(h, on), h)
        assert helm_lib.helm_get_transposed(h) == 1 - on          # in force from the next assembly only
        _lib.check(helm_lib.helm_assemble(h, f.real, f.imag, float(tr.tau), 0.0, float(tr.cPML)), h)
        assert helm_lib.helm_get_transposed(h) == on
        _lib.check(helm_lib.helm_get_block_diagonals(h, 0, _lib.ptr(out)), h)
        assert np.array_equal(bits(out), bits(want))
    del plain.factors, tr.factors


def test_refusals_of_the_entry_point_and_of_a_transposed_handle(helm_lib):
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = ec.operator_config('20x24', 'vti')
    # eps != delta: the coupled system
    e2 = np.array(sc['eps'])
    e2[3, 4] += 0.01
    coupled = za.Eurus(dict(sc, eps=e2))
    assert helm_lib.helm_set_transposed_m1(coupled.handle, 1) == -4
    assert 'coupled' in _lib.last_error(coupled.handle)
    mz = za.MiniZephyr(dict(sc))
    assert helm_lib.helm_set_transposed_m1(mz.handle, 1) == -4
    assert helm_lib.helm_set_transposed_m1(None, 1) == -1
    plain = za.Eurus(sc)
    assert helm_lib.helm_set_transposed(plain.handle, 1) == -4 and 'MiniZephyr' in _lib.last_error(plain.handle)          # (as it always was)
    # a transposed handle: N-row right-hand sides through the direct path, nothing else
    tr = za.Eurus(dict(sc, transposed=True))
    N = tr.nrow
    q = randc(np.random.default_rng(1), (N, 2))
    assert np.all(np.isfinite(tr * q))
    with pytest.raises(_lib.HelmError) as ei:
        tr * np.vstack([q, q])
    assert 'M1^T' in str(ei.value) and '2N' in str(ei.value)
    out = np.empty((9, 24, 20), dtype=np.complex128)
    assert helm_lib.helm_get_block_diagonals(tr.handle, 1, _lib.ptr(out)) == -4
    big = np.empty((4, 9, 24, 20), dtype=np.complex128)
    assert helm_lib.helm_get_diagonals(tr.handle, _lib.ptr(big)) == -4
    kr = za.Eurus(dict(sc, transposed=True, method='bicgstab'))
    with pytest.raises(_lib.HelmError) as ei:
        kr * q
    assert 'Krylov' in str(ei.value)
    for o in (coupled, mz, plain, tr, kr):
        del o.factors


# ---- 2. the transposed solve against SuperLU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aniso', ec.ANISO)
@pytest.mark.parametrize('cls', ['Eurus', 'EurusHD'])
@pytest.mark.parametrize('grid', ['20x24', '96x80'])
def test_transposed_solve_matches_superlu_and_differs_from_the_plain_one(helm_lib, grid, cls, aniso):
    "the tolerances of tests/test_gpu_adjoint.py for MiniZephyr: rel-L2 1e-7 against splu(M1).solve(trans='T'), every relres within rtol = 1e-10"
    import zephyr_amd as za
    sc = ec.operator_config(grid, aniso, freq=20., rtol=1e-10, method='direct')
    tr, plain = getattr(za, cls)(dict(sc, transposed=True)), getattr(za, cls)(sc)
    nz, nx = sc['nz'], sc['nx']
    rng = np.random.default_rng(2)
    X, Z = 10. * (nx - 1), 8. * (nz - 1)
    locs = np.stack([rng.uniform(0.3 * X, 0.7 * X, 3), rng.uniform(0.3 * Z, 0.7 * Z, 3)], axis=1)
    lu = spla.splu(ho.coefficients_to_csr(ec.oracle_c4(plain)[0]).tocsc())
    for q in (za.SparseKaiserSource(sc)(locs), randc(rng, (nz * nx, 5))):
        qd = q.toarray() if hasattr(q, 'toarray') else np.asarray(q)
        u = tr * q
        info = tr.lastInfo
        ref = np.conj(lu.solve(complex(tr.premul) * np.asarray(qd, dtype=np.complex128), trans='T'))
        err = rel(u, ref)
        print('%s %s %s: transposed solve against SuperLU rel-L2 %.2e, worst relres %.2e' % (grid, cls, aniso, err, max(i['relres'] for i in info)))
        assert err <= 1e-7, info
        assert all(i['relres'] <= 1e-10 for i in info), info
        assert rel(plain * q, u) > 1e-3                                 # (a model on which M1^-T and M1^-1 differ: otherwise this shows nothing)
    del tr.factors, plain.factors


# ---- 3. the kernels against the 80-bit host evaluation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aniso', ec.ANISO)
@pytest.mark.parametrize('grid', ['20x24', '37x53', '70x67'])
def test_planes_and_adjoint_kernels_against_the_80_bit_evaluation(helm_lib, grid, aniso):
    """dC = V[dc] + L[db] (both, and each alone) and Gc += w V^T P, Gb += w L^T P (both outputs, and each alone; plain and conjugated) per component within
    C_EU_PLANES, C_EU_ADJOINT_C and C_EU_ADJOINT_B times 2^-53 of the magnitudes of eurus_cases; guard cells stay, G starts non-zero, two runs give the same
    bits, one output alone gives the bits it has beside the other."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    sc = ec.operator_config(grid, aniso, tau=0.4 if grid == '37x53' else np.inf)
    op = za.Eurus(dict(sc, device=0))
    dc, db, Pl, G0c, G0b = ec.kernel_inputs(sc)
    N = dc.size
    dev = torch.device('cuda', 0)
    guard, fill = 517, complex(7.0, -3.0)
    dDc, dDb, dP = (torch.from_numpy(a).to(dev) for a in (dc, db, Pl))
    worst = {}
    for name, a, b in (('planes', dc, db), ('planes dc', dc, None), ('planes db', None, db)):
        runs = []
        for _ in range(2):
            out = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
            torch.cuda.synchronize(dev)
            d_c = P(out.data_ptr() + 16 * guard)
            _lib.check(helm_lib.helm_eurus_planes_device(op.handle, None if a is None else P(dDc.data_ptr()), None if b is None else P(dDb.data_ptr()), d_c), op.handle)
            h = out.cpu().numpy()
            assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
            runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
        assert np.array_equal(bits(runs[0]), bits(runs[1]))
        ref, mag = ec.planes_reference(op, a, b)
        worst[name] = ec.worst_ratio(runs[0], ref, ec.C_EU_PLANES * ec.U64 * mag)
        edge = ~np.asarray(ec.fr._interiorMask(sc['nz'], sc['nx'])).ravel()
        assert np.all(runs[0][:4, edge] == 0) and np.all(runs[0][5:, edge] == 0) and np.all(runs[0][4, edge] != 0)
    w = -0.7 + 0.4j
    for conj in (0, 1):
        (refc, magc), (refb, magb) = ec.adjoint_reference(op, G0c, G0b, Pl, w, bool(conj))
        got = {}
        for which in ('both', 'c', 'b'):
            runs = []
            for _ in range(2 if which == 'both' else 1):
                bufc, bufb = (torch.full((2 * guard + N,), fill, dtype=torch.complex128, device=dev) for _ in range(2))
                bufc[guard:guard + N], bufb[guard:guard + N] = torch.from_numpy(G0c).to(dev), torch.from_numpy(G0b).to(dev)
                torch.cuda.synchronize(dev)
                d_gc = P(bufc.data_ptr() + 16 * guard) if which in ('both', 'c') else None
                d_gb = P(bufb.data_ptr() + 16 * guard) if which in ('both', 'b') else None
                _lib.check(helm_lib.helm_eurus_adjoint_device(op.handle, P(dP.data_ptr()), w.real, w.imag, conj, d_gc, d_gb), op.handle)
                hc, hb = bufc.cpu().numpy(), bufb.cpu().numpy()
                for hh in (hc, hb):
                    assert np.all(hh[:guard] == fill) and np.all(hh[guard + N:] == fill)
                runs.append((hc[guard:guard + N].copy(), hb[guard:guard + N].copy()))
            if which == 'both':
                assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(*runs))
            got[which] = runs[0]
        assert np.array_equal(bits(got['c'][0]), bits(got['both'][0])) and np.array_equal(bits(got['c'][1]), bits(G0b))          # (the output not asked for stays)
        assert np.array_equal(bits(got['b'][1]), bits(got['both'][1])) and np.array_equal(bits(got['b'][0]), bits(G0c))
        worst['adjoint c conj=%d' % conj] = ec.worst_ratio(got['both'][0], refc, ec.C_EU_ADJOINT_C * ec.U64 * magc)
        worst['adjoint b conj=%d' % conj] = ec.worst_ratio(got['both'][1], refb, ec.C_EU_ADJOINT_B * ec.U64 * magb)
    print('%s %s: worst err / bound %s' % (grid, aniso, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert all(x <= 1.0 for x in worst.values()), worst
    # bad arguments are refused before anything is launched; a MiniZephyr handle and a coupled model are not served
    assert helm_lib.helm_eurus_planes_device(op.handle, P(dDc.data_ptr() + 4), None, d_c) == -1
    assert helm_lib.helm_eurus_adjoint_device(op.handle, P(dP.data_ptr()), 1.0, 0.0, 0, None, None) == -1
    assert helm_lib.helm_eurus_adjoint_device(op.handle, P(dP.data_ptr()), 1.0, 0.0, 0, P(dP.data_ptr() + 16), None) == -1
    if grid == '20x24':
        mz = za.MiniZephyr(dict(sc, device=0))
        assert helm_lib.helm_eurus_planes_device(mz.handle, P(dDc.data_ptr()), None, d_c) == -4
        assert helm_lib.helm_eurus_adjoint_device(mz.handle, P(dP.data_ptr()), 1.0, 0.0, 0, P(bufc.data_ptr()), None) == -4
        del mz.factors
    del op.factors


@pytest.mark.parametrize('fmt', ['complex128', 'complex64'])
@pytest.mark.parametrize('grid', ['20x24', '37x53', '70x67'])
def test_centre_edges_kernel_against_the_80_bit_evaluation(helm_lib, grid, fmt):
    """P_4 += sum_s UB_s UF_s on the boundary cells per component within (2 nsrc + 1) 2^-53 (+ 2^-24 for the complex64 store) of the magnitude; every other entry
    of P and the guard cells keep their bits; leading dimensions > N; two runs give the same bits."""
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import pack_reference
    nz, nx, _ = ec.GRIDS[grid]
    nsrc = 5
    op = za.Eurus(dict(ec.operator_config(grid, 'iso'), device=0))
    op.handle
    dev = torch.device('cuda', 0)
    N = nz * nx
    rng = np.random.default_rng(nz + nx)
    U, B, P0 = randc(rng, (nsrc, N)) * 10. ** rng.uniform(-3, 3, (nsrc, 1)), randc(rng, (nsrc, N)), randc(rng, (9, N))
    ldu, ldb, guard, fill = N + 38, N + 5, 517, complex(7.0, -3.0)
    fterm = 2.0 ** -24 if fmt == 'complex64' else 0.0
    Bpad = np.zeros((nsrc, ldb), dtype=np.complex128)
    Bpad[:, :N] = B
    dB = torch.from_numpy(Bpad).to(dev)
    if fmt == 'complex64':
        Pk, e = pack_reference(np.ascontiguousarray(U.T))
        Ppad = np.zeros((nsrc, ldu), dtype=np.complex64)
        Ppad[:, :N] = Pk.T
        dU, dE = torch.from_numpy(Ppad).to(dev), torch.from_numpy(e).to(dev)
    else:
        Upad = np.zeros((nsrc, ldu), dtype=np.complex128)
        Upad[:, :N] = U
        dU, dE = torch.from_numpy(Upad).to(dev), None
    runs = []
    for _ in range(2):
        buf = torch.full((2 * guard + 9 * N,), fill, dtype=torch.complex128, device=dev)
        buf[guard:guard + 9 * N] = torch.from_numpy(P0.ravel()).to(dev)
        torch.cuda.synchronize(dev)
        d_p = P(buf.data_ptr() + 16 * guard)
        if fmt == 'complex64':
            _lib.check(helm_lib.helm_lag_centre_edges_accumulate_c64_device(op.handle, P(dU.data_ptr()), P(dE.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, d_p), op.handle)
        else:
            _lib.check(helm_lib.helm_lag_centre_edges_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, nsrc, d_p), op.handle)
        h = buf.cpu().numpy()
        assert np.all(h[:guard] == fill) and np.all(h[guard + 9 * N:] == fill)
        runs.append(h[guard:guard + 9 * N].reshape((9, N)).copy())
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    ref, mag = ec.edges_reference(P0, U, B, nz, nx)
    worst = ec.worst_ratio(runs[0], ref, (ec.c_edges(nsrc) * ec.U64 + fterm) * mag)
    print('%s %s: centre edges worst err / bound %.3f' % (grid, fmt, worst))
    assert worst <= 1.0
    edge = ~np.asarray(ec.fr._interiorMask(nz, nx)).ravel()
    untouched = np.ones((9, N), dtype=bool)
    untouched[4, edge] = False
    assert np.array_equal(bits(runs[0][untouched]), bits(P0[untouched]))
    assert helm_lib.helm_lag_centre_edges_accumulate_device(op.handle, P(dU.data_ptr()), N - 1, P(dB.data_ptr()), ldb, nsrc, d_p) == -1
    assert helm_lib.helm_lag_centre_edges_accumulate_device(op.handle, P(dU.data_ptr()), ldu, P(dB.data_ptr()), ldb, 0, d_p) == -1
    del op.factors


# ---- 4. the device routes against the host route ----------------------------------------------------------------------------------------------------------
ROUTES = [('fixed', False, 'complex128', True), ('relative', True, 'complex64', True), ('fixed', True, 'complex128', False)]          # mode, HD class, store, explicit rho


def _inputs(prob, sv):
    rng = np.random.default_rng(31)
    vc, vr = ec.perturbations(prob.nrow)
    return vc, vr, np.concatenate((vc, vr)), randc(rng, sv.nD)


@pytest.mark.parametrize('mode,hd,fmt,density', ROUTES, ids=['%s-%s-%s-%s' % (r[0], 'hd' if r[1] else 'eu', r[2], 'rho' if r[3] else 'gardner') for r in ROUTES])
def test_device_routes_against_the_host_routes_on_the_downloaded_fields(helm_lib, monkeypatch, mode, hd, fmt, density):
    """Jtvec, JvecBorn and Hvec with u = F for 'c', 'rho' and 'joint' ('full'; and the 'scaler' pair) within 1e-6 of the numpy routes fed the downloaded fields --
    the tolerance of tests/test_gpu_joint.py and tests/test_gpu_full.py: two solves at rtol 1e-11 on either side; the joint halves against the single-parameter
    device calls; the same bits from a second call and (complex128 store) from u = None."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = ec.device_pair(mode, hd, density=density, rtol=1e-11, **({} if fmt == 'complex128' else dict(fieldsDtype=fmt)))
    assert prob._deviceGradientAvailable()
    N = prob.nrow
    vc, vr, v, r = _inputs(prob, sv)
    F = prob.fieldsDevice()
    assert F.dtype == fmt
    host = list(F)
    combos = [('scaler', 'c', vc), ('full', 'c', vc)] + ([('full', 'rho', vr), ('operator', 'joint', v), ('full', 'joint', v)] if density else [])
    err, got = {}, {}
    for lin, par, x in combos:
        kw = dict(linearisation=lin, parameter=par)
        calls = {'Jtvec': lambda u: prob.Jtvec(None, r, u=u, adjoint='transpose', **kw), 'JvecBorn': lambda u: prob.JvecBorn(None, x, u=u, **kw),
                 'Hvec': lambda u: prob.Hvec(None, x, u=u, **kw)}
        for name, call in calls.items():
            g = call(F)
            got[name, lin, par] = g
            err['%s %s %s' % (name, lin, par)] = rel(g, call(host))
            assert np.array_equal(bits(call(F)), bits(g)), (name, lin, par)
            if fmt == 'complex128':
                assert np.array_equal(bits(call(None)), bits(g)), (name, lin, par)
        lhs = inner(got['JvecBorn', lin, par], r)
        assert abs(lhs - inner(x, got['Jtvec', lin, par])) <= 1e-7 * abs(lhs)          # (the identity through the device routes: tests/test_gpu_adjoint.py)
    print('%s %s %s %s: device against host %s' % (mode, hd, fmt, density, {k: '%.1e' % e for k, e in err.items()}))
    assert all(e <= 1e-6 for e in err.values()), err
    if density:
        gj = got['Jtvec', 'full', 'joint']
        assert gj.shape == (2 * N,) and gj.dtype == np.float64
        assert rel(gj[:N], got['Jtvec', 'full', 'c']) <= 1e-6 and rel(gj[N:], got['Jtvec', 'full', 'rho']) <= 1e-6
        assert np.array_equal(bits(got['Jtvec', 'operator', 'joint']), bits(gj))          # (on Eurus 'operator' and 'full' are the same derivative)
        assert rel(got['JvecBorn', 'full', 'joint'], got['JvecBorn', 'full', 'c'] + got['JvecBorn', 'full', 'rho']) <= 1e-6
    with pytest.raises(NotImplementedError, match='Eurus'):
        prob.Hvec(None, vc, u=F, linearisation='full', resid=r)
    F.release()
    del prob.factors


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    "two workers on GPU 0 with half the sources each: the stacked partials are added on the host"
    import zephyr_amd as za
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    sc = ec.survey_config('fixed', True, Disc=za.EurusHD, freqs=[ec.FREQS[1]], sterms=np.array([0.8 - 0.3j]), rtol=1e-11)
    del sc['parallel']                                                                                    # (the workers of HELM_DEVICES)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    assert len(prob.system.devices) == 2
    _, _, v, r = _inputs(prob, sv)
    F = prob.fieldsDevice()
    assert len(F.items) == 2
    kw = dict(linearisation='full', parameter='joint')
    assert rel(prob.Jtvec(None, r, u=F, adjoint='transpose', **kw), prob.Jtvec(None, r, u=[F[0]], adjoint='transpose', **kw)) <= 1e-6
    assert rel(prob.JvecBorn(None, v, u=F, **kw), prob.JvecBorn(None, v, u=[F[0]], **kw)) <= 1e-6
    host = prob.Hvec(None, v, u=[F[0]], **kw)
    for H in (prob.Hvec(None, v, u=F, **kw), prob.Hvec(None, v, **kw)):
        assert rel(H, host) <= 1e-6
    F.release()
    del prob.factors


# ---- 5. Taylor at the level of dpred, through the device routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('top', [False, True], ids=['sources-inside', 'sources-on-the-top-line'])
def test_taylor_remainder_of_dpred_through_the_device_routes(helm_lib, monkeypatch, top):
    "dpred and JvecBorn(u=F, 'full', 'joint') on the GPU operators: every factor of the remainder over h = 1, 1/2, 1/4, 1/8 in the second-order window"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv = ec.device_pair('relative' if not top else 'fixed', not top, top_source=top, rtol=1e-11)
    c0, rho0 = np.array(prob.systemConfig['c']), np.array(prob.systemConfig['rho'])
    vc, vr, v, _ = _inputs(prob, sv)
    F = prob.fieldsDevice()
    Jv = prob.JvecBorn(None, v, u=F, linearisation='full', parameter='joint')
    F.release()
    d0 = sv.dpred({'c': np.array(c0), 'rho': np.array(rho0)})
    rem = [ec.fc.norm(sv.dpred({'c': c0 + h * vc.reshape(c0.shape), 'rho': rho0 + h * vr.reshape(c0.shape)}) - d0 - h * Jv) for h in ec.fc.TAYLOR_H]
    f = ec.fc.factors(rem)
    print('device Taylor (%s): remainders %s factors %s' % ('top line' if top else 'inside', rem, f))
    assert all(x >= ec.SECOND for x in f)
    del prob.factors


# ---- 6. what exists stays as it is -----------------------------------------------------------------------------------------------------------------------------
def test_minizephyr_and_keyless_eurus_give_the_same_bits_before_and_after_an_eurus_derivative_call(helm_lib, monkeypatch):
    import zephyr_amd as za
    from zephyr_amd import _lib
    from tests import full_cases as xc
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0')

    def minizephyr():
        prob, sv = xc.pair('fixed', False, device=True, rtol=1e-11)
        rng = np.random.default_rng(41)
        v, r = rng.standard_normal(prob.nrow), randc(rng, sv.nD)
        out = [prob.JvecBorn(None, v, linearisation='full'), prob.Jtvec(None, r, adjoint='transpose', linearisation='full'), sv.dpred(None)]
        del prob.factors
        return out

    def keyless():
        sc = ec.survey_config('fixed', False, Disc=za.Eurus, rtol=1e-11)
        del sc['eurusDerivatives']
        prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
        prob.pair(sv)
        r = randc(np.random.default_rng(42), sv.nD)
        out = [sv.dpred(None), prob.Jtvec(None, r)]
        with pytest.raises(NotImplementedError, match='has no transposed operator: helm_set_transposed serves 2-D MiniZephyr handles'):
            prob.Jtvec(None, r, adjoint='transpose')
        with pytest.raises(NotImplementedError, match='assembles its mass term differently'):
            prob.JvecBorn(None, np.ones(prob.nrow), linearisation='full')
        # the C return codes of the entry points that refuse an Eurus handle
        import torch
        op = prob.system.subProblems[0]
        N = op.nrow
        u, c9 = torch.zeros(N, dtype=torch.complex128, device='cuda'), torch.zeros(9 * N, dtype=torch.complex128, device='cuda')
        torch.cuda.synchronize()
        assert helm_lib.helm_stencil_sources_device(op.handle, P(u.data_ptr()), 1, N, P(c9.data_ptr()), 1.0, 0.0, 0, P(c9.data_ptr() + 16 * N), N) == -4
        assert helm_lib.helm_lag_imaging_accumulate_device(op.handle, P(u.data_ptr()), N, P(c9.data_ptr() + 16 * N), N, 1, P(c9.data_ptr() + 32 * N)) == -4
        assert helm_lib.helm_set_transposed(op.handle, 1) == -4
        del prob.factors
        return out

    before = minizephyr() + keyless()
    prob, sv = ec.device_pair('fixed', False, rtol=1e-11)
    _, _, v, r = _inputs(prob, sv)
    prob.Hvec(None, v, linearisation='full', parameter='joint')
    prob.Jtvec(None, r, adjoint='transpose', linearisation='full', parameter='joint')
    del prob.factors
    after = minizephyr() + keyless()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
