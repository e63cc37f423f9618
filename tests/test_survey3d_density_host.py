"""CPU: the buoyancy derivative of the 3-D operator without a GPU -- the host maps of frechet3d.py against two oracle matrices, and the routes that
derivatives3D=True opens on Helm3DProblem (parameter 'rho' and 'joint', the Gardner total derivative, Hvec) on the splu-backed stand-in of
tests/survey3d_cases.py: adjoint identities, Taylor remainders, the joint routes against the single-parameter ones, and every refusal."""
import numpy as np
import pytest
import scipy.sparse as sp

import zephyr_amd as za
from zephyr_amd import frechet3d
from tests import survey3d_cases as s3
from tests import survey3d_density_cases as d3c

_PAIRS = {}
CASES = [('12x11x13', 'fixed'), ('12x11x13', 'relative'), ('18x16x20', 'fixed')]
T = dict(adjoint='transpose')


def pair(grid, mode='fixed', gardner=False):
    'one problem / survey pair per case for the whole module: the LU factors of the base model are made once'
    key = (grid, mode, gardner)
    if key not in _PAIRS:
        prob, sv = d3c.host_pair(grid, mode, gardner)
        _PAIRS[key] = (prob, sv, np.array(prob.systemConfig['c']), None if gardner else np.array(prob.systemConfig['rho']))
    return _PAIRS[key]


def kinds(grid, mode):
    "the three derivatives: (label, pair, keywords, size of v, m(h, v) -> the model moved by h v)"
    prob, sv, c0, rho0 = pair(grid, mode)
    pg, sg, cg, _ = pair(grid, mode, gardner=True)
    N = prob.nrow
    return [('rho', (prob, sv), dict(linearisation='operator', parameter='rho'), N, lambda h, v: dict(c=c0, rho=rho0 + h * v.reshape(c0.shape))),
            ('joint', (prob, sv), dict(linearisation='full', parameter='joint'), 2 * N,
             lambda h, v: dict(c=c0 + h * v[:N].reshape(c0.shape), rho=rho0 + h * v[N:].reshape(c0.shape))),
            ('gardner', (pg, sg), dict(linearisation='full', parameter='c'), N, lambda h, v: cg + h * v.reshape(cg.shape))]


# ---- 1. the formula ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['12x11x13', '18x16x20'])
def test_buoyancy_maps_are_the_difference_of_two_oracle_matrices(grid):
    "dA[db] = 1/2 diag(db) L + 1/2 L diag(db) + M~ diag(kappa db) against oracle_matrix(b + db) - oracle_matrix(b): the row is linear in b, so only rounding separates them"
    prob, sv, c0, rho0 = pair(grid)
    op = prob.system.subProblems[0]
    rng = np.random.default_rng(4)
    b = 1.0 / rho0.ravel()
    db = 1e-4 * b * rng.uniform(0.5, 1.0, b.size)
    base = dict(prob.systemConfig, freq=sv.freqs[0])
    A0 = s3.oracle_matrix(s3.OracleHelm3D(base))
    A1 = s3.oracle_matrix(s3.OracleHelm3D(dict(base, rho=(1.0 / (b + db)).reshape(rho0.shape))))
    L, M = frechet3d.lapStencil3(op), frechet3d.massStencil3(op.modelDims)
    want = 0.5 * sp.diags(db) @ L + 0.5 * L @ sp.diags(db) + M @ sp.diags(frechet3d.kappa3(op) * db)
    err, floor = abs((A1 - A0) - want).max(), d3c.fd_floor(op, L, b + db)
    print('%s: |A(b + db) - A(b) - dA[db]|max = %.2e, floor %.2e, |dA|max = %.2e (relative %.2e)' % (grid, err, floor, abs(want).max(), err / abs(want).max()))
    assert err <= floor
    assert floor <= 1e-9 * abs(want).max()                               # (and the floor is a check: ten digits of dA)
    # L is far from symmetric on its own scale: no "symmetric" shortcut can stand in for L^T
    asym = abs(L - L.T).max() / abs(L).max()
    print('%s: |L - L^T|max / |L|max = %.3f' % (grid, asym))
    assert asym >= 0.1
    inside = frechet3d.interiorMask3(op.modelDims)
    assert np.all(np.diff(L.indptr)[inside] == 27) and np.all(np.diff(L.indptr)[~inside] == 0)
    # the columns of buoyancySources3 are that matrix applied, the boundary rows exact zeros
    uh = s3.randc(rng, (op.nrow, 2))
    q = frechet3d.buoyancySources3(op, db, uh, L, M)
    assert s3.rel(q, want @ uh) <= 1e-14 and np.all(q[~inside] == 0)
    assert np.allclose(frechet3d.kappa3(op) * b, frechet3d.massField3(op), rtol=1e-14, atol=0)
    assert np.array_equal(frechet3d.densityChain3(op), -1.0 / rho0.ravel() ** 2)


def test_gardner_chain_is_the_derivative_of_the_default_density():
    pg, sg, cg, _ = pair('12x11x13', gardner=True)
    op = pg.system.subProblems[0]
    assert np.allclose(1.0 / np.asarray(op.rho).ravel(), cg.ravel() ** -0.25 / 310., rtol=1e-15)
    h = 1e-3
    fd = ((cg.ravel() + h) ** -0.25 - (cg.ravel() - h) ** -0.25) / (310. * 2 * h)
    assert np.allclose(frechet3d.gardnerChain3(op), fd, rtol=1e-8, atol=0)            # (central difference: O(h^2 / c^2) = 3e-13, its rounding u c / h = 2e-10)


# ---- 2. the adjoint identity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid,mode', CASES)
def test_adjoint_identity_of_the_density_joint_and_gardner_routes(grid, mode, monkeypatch):
    for label, (prob, sv), kw, n, _ in kinds(grid, mode):
        rng = np.random.default_rng(8)
        v = rng.standard_normal(n)
        r = s3.randc(rng, sv.nD)
        Jv = prob.JvecBorn(None, v, **kw)
        g = prob.Jtvec(None, r, **T, **kw)
        assert g.dtype == np.float64 and g.shape == (n,)
        lhs, rhs = s3.inner(r, Jv), float(g @ v)
        miss = abs(lhs - rhs) / abs(lhs)
        print('%s %s %s: adjoint identity misses by %.2e' % (grid, mode, label, miss))
        assert miss <= 1e-12
        F = prob.fields(None)
        assert s3.rel(prob.Jtvec(None, r, u=F, **T, **kw), g) <= 1e-12 and s3.rel(prob.JvecBorn(None, v, u=F, **kw), Jv) <= 1e-13
        # the counter-test: L in the place of L^T in the imaging map is not the adjoint
        real = frechet3d.buoyancyImaging3
        monkeypatch.setattr(frechet3d, 'buoyancyImaging3', lambda op, uh, lam, L=None, M=None: real(op, uh, lam, L, M, LT=L))
        gw = prob.Jtvec(None, r, u=F, **T, **kw)
        monkeypatch.setattr(frechet3d, 'buoyancyImaging3', real)
        wrong = abs(lhs - float(gw @ v)) / abs(lhs)
        print('%s %s %s: with L in the place of L^T the identity misses by %.2e' % (grid, mode, label, wrong))
        assert wrong > 1e-3


# ---- 3. Taylor remainders ---------------------------------------------------------------------------------------------------------------------------------
def perturbation(rng, label, n, N):
    'non-zero everywhere -- boundary nodes and the absorbing layers included --, in the units of the parameter'
    v = rng.uniform(0.3, 1., n) * rng.choice([-1., 1.], n)
    scale = dict(rho=60., gardner=40.)
    return v * scale[label] if label in scale else np.concatenate([40. * v[:N], 60. * v[N:]])


@pytest.mark.parametrize('grid,mode', CASES)
def test_taylor_remainders_along_density_joint_and_gardner(grid, mode, monkeypatch):
    for label, (prob, sv), kw, n, moved in kinds(grid, mode):
        v = perturbation(np.random.default_rng(7), label, n, prob.nrow)
        assert np.all(v != 0)
        d0 = sv.dpred(moved(0., v))
        J = prob.JvecBorn(None, v, **kw)
        # the same call with the Laplacian part left out of the Born sources: the kappa term alone
        real = frechet3d.lapStencil3
        monkeypatch.setattr(frechet3d, 'lapStencil3', lambda op: 0.0 * real(op))
        Jk = prob.JvecBorn(None, v, **kw)
        monkeypatch.setattr(frechet3d, 'lapStencil3', real)
        rem, remk = [], []
        for j in range(6):
            h = 0.5 ** j
            d = sv.dpred(moved(h, v))
            rem.append(np.linalg.norm(d - d0 - h * J))
            remk.append(np.linalg.norm(d - d0 - h * Jk))
        prob.updateModel(moved(0., v))
        ratios = [rem[j] / rem[j + 1] for j in range(5)]
        stalled = [remk[j] / remk[j + 1] for j in range(5)]
        print('%s %s %s: Taylor remainders %s, ratios %s; without the Laplacian part %s' % (grid, mode, label, ['%.3e' % x for x in rem], ['%.3f' % x for x in ratios],
                                                                                         ['%.3f' % x for x in stalled]))
        assert all(3.9 <= x <= 4.1 for x in ratios), (label, ratios)
        assert rem[0] > 1e-3 * np.linalg.norm(J)
        assert all(x < 3. for x in stalled), (label, stalled)


# ---- 4. joint, Hvec -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid,mode', CASES[:2])
def test_joint_is_the_two_single_parameter_calls_and_hvec_is_the_composition(grid, mode):
    prob, sv, c0, rho0 = pair(grid, mode)
    N = prob.nrow
    rng = np.random.default_rng(12)
    v, w, r = rng.standard_normal(2 * N), rng.standard_normal(2 * N), s3.randc(rng, sv.nD)
    v[N:] *= 0.5
    F = prob.fields(None)
    O = dict(linearisation='operator')
    g = prob.Jtvec(None, r, u=F, **T, **O, parameter='joint')
    gc, gr = prob.Jtvec(None, r, u=F, **T, **O), prob.Jtvec(None, r, u=F, **T, **O, parameter='rho')
    assert g.shape == (2 * N,) and s3.rel(g[:N], gc) <= 1e-12 and s3.rel(g[N:], gr) <= 1e-12
    J = prob.JvecBorn(None, v, u=F, **O, parameter='joint')
    Jc, Jr = prob.JvecBorn(None, v[:N], u=F, **O), prob.JvecBorn(None, v[N:], u=F, **O, parameter='rho')
    assert s3.rel(J, Jc + Jr) <= 1e-12
    # the model as a dict is the model as it stands
    assert s3.rel(prob.Jtvec(dict(c=c0, rho=rho0), r, **T, **O, parameter='joint'), g) <= 1e-12
    # Hvec: the hand composition, symmetric, positive, and its blocks
    wts = rng.uniform(0.5, 2., sv.nD)
    Hv = prob.Hvec(None, v, u=F, **O, parameter='joint')
    assert Hv.dtype == np.float64 and s3.rel(Hv, prob.Jtvec(None, J, u=F, **T, **O, parameter='joint')) <= 1e-13
    Hw = prob.Hvec(None, w, u=F, **O, parameter='joint')
    sym = abs(float(Hv @ w) - float(v @ Hw)) / abs(float(Hv @ w))
    print('%s %s: <Hv, w> against <v, Hw> misses by %.2e; <v, Hv> = %.3e' % (grid, mode, sym, float(v @ Hv)))
    assert sym <= 1e-12 and float(v @ Hv) > 0
    assert s3.rel(prob.Hvec(None, v, u=F, weights=wts, **O, parameter='joint'), prob.Jtvec(None, J * wts, u=F, **T, **O, parameter='joint')) <= 1e-13
    p0 = np.concatenate([v[:N], np.zeros(N)])
    H0 = prob.Hvec(None, p0, u=F, **O, parameter='joint')
    assert s3.rel(H0[:N], prob.Hvec(None, v[:N], u=F, **O, parameter='c')) <= 1e-12
    assert s3.rel(H0[N:], prob.Jtvec(None, Jc, u=F, **T, **O, parameter='rho')) <= 1e-12
    assert s3.rel(prob.Hvec(None, v[N:], u=F, **O, parameter='rho'), prob.Jtvec(None, Jr, u=F, **T, **O, parameter='rho')) <= 1e-13
    assert s3.rel(prob.Hvec(None, v, **O, parameter='joint'), Hv) <= 1e-12                   # u None: the fields are solved once for both halves
    # the Gardner product
    pg, sg, cg, _ = pair(grid, mode, gardner=True)
    G = dict(linearisation='full')
    Hg = pg.Hvec(None, v[:N], **G)
    assert s3.rel(Hg, pg.Jtvec(None, pg.JvecBorn(None, v[:N], **G), **T, **G)) <= 1e-12 and float(v[:N] @ Hg) > 0


def test_a_density_change_rebuilds_both_wrappers():
    prob, sv = d3c.host_pair('12x11x13')
    c0, rho0 = np.array(prob.systemConfig['c']), np.array(prob.systemConfig['rho'])
    r = s3.randc(np.random.default_rng(2), sv.nD)
    kw = dict(adjoint='transpose', linearisation='operator', parameter='joint')
    g0 = prob.Jtvec(None, r, **kw)
    sys0, adj0 = prob.system, prob.adjointSystem
    g1 = prob.Jtvec(dict(c=c0, rho=1.05 * rho0), r, **kw)
    assert prob.system is not sys0 and prob.adjointSystem is not adj0
    assert np.array_equal(prob.adjointSystem.subProblems[0].rho, 1.05 * rho0) and s3.rel(g1, g0) > 1e-3
    fresh, _ = d3c.host_pair('12x11x13', rho=1.05 * rho0)
    assert s3.rel(g1, fresh.Jtvec(None, r, **kw)) <= 1e-12


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_without_the_key_everything_is_refused_as_before():
    prob, sv = s3.host_pair('12x11x13')
    c0 = np.array(prob.systemConfig['c'])
    r, v = np.zeros(sv.nD, dtype=complex), np.zeros(prob.nrow)
    norho = dict(prob.systemConfig)
    del norho['rho']
    p2, s2 = za.Helm3DProblem(norho), za.Helm3DSurvey(norho)
    p2.pair(s2)
    for call in (lambda: p2.Jtvec(c0, r, adjoint='transpose', linearisation='operator'), lambda: p2.JvecBorn(c0, v, linearisation='full')):
        with pytest.raises(NotImplementedError, match=r'(?s)rho.*Gardner.*Laplacian.*that derivative is not built'):
            call()
    for par in ('rho', 'joint', 'Q'):
        with pytest.raises(NotImplementedError, match='the density, joint and Q derivatives exist for the 2-D operators only'):
            prob.Jtvec(c0, r, adjoint='transpose', linearisation='operator', parameter=par)
        with pytest.raises(NotImplementedError, match="parameter='c'"):
            prob.JvecBorn(c0, v, linearisation='operator', parameter=par)
    with pytest.raises(NotImplementedError, match=r'(?s)Hvec.*Jtvec\(JvecBorn'):
        prob.Hvec(c0, v)
    with pytest.raises(NotImplementedError, match='no density derivative in 3-D'):
        prob.hessianBlocks(c0)


def test_with_the_key_what_stays_refused_says_why():
    prob, sv, c0, rho0 = pair('12x11x13')
    pg, sg, cg, _ = pair('12x11x13', gardner=True)
    N = prob.nrow
    r, v = np.zeros(sv.nD, dtype=complex), np.zeros(N)
    X = dict(adjoint='transpose', linearisation='operator')
    for par in ('Q', 'cQ'):
        with pytest.raises(NotImplementedError, match=r'(?s)not built in 3-D.*\(c, Q\)'):
            prob.Jtvec(None, r, parameter=par, **X)
        with pytest.raises(NotImplementedError, match=r'(?s)not built in 3-D.*\(c, Q\)'):
            prob.JvecBorn(None, v, linearisation='full', parameter=par)
        with pytest.raises(NotImplementedError, match='not built in 3-D'):
            prob.Hvec(None, v, parameter=par)
    with pytest.raises(ValueError, match="'c' or 'rho'"):
        prob.Jtvec(None, r, parameter='vp', **X)
    for par in ('rho', 'joint'):
        with pytest.raises(ValueError, match="needs linearisation='operator'"):
            prob.Jtvec(None, r, adjoint='transpose', linearisation='scaler', parameter=par)
    with pytest.raises(ValueError, match="adjoint='transpose'"):
        prob.Jtvec(None, r, linearisation='operator', parameter='rho')
    with pytest.raises(ValueError, match='stacked vector'):
        prob.JvecBorn(None, v, linearisation='operator', parameter='joint')
    with pytest.raises(ValueError, match='stacked vector'):
        prob.Hvec(None, v, parameter='joint')
    # the Gardner density: 'full' for 'c' alone
    for kw in (dict(linearisation='operator'), dict(linearisation='full', parameter='rho'), dict(linearisation='full', parameter='joint')):
        with pytest.raises(NotImplementedError, match=r"(?s)without `rho`.*linearisation='full', parameter='c'.*Gardner"):
            pg.Jtvec(None, r, adjoint='transpose', **kw)
        with pytest.raises(NotImplementedError, match=r'(?s)without `rho`.*Gardner'):
            pg.JvecBorn(None, np.zeros(2 * N if kw.get('parameter') == 'joint' else N), **kw)
        with pytest.raises(NotImplementedError, match=r'(?s)without `rho`.*Gardner'):
            pg.Hvec(None, v, **kw)
    # Hvec: the Newton term and 'scaler'
    with pytest.raises(NotImplementedError, match=r'(?s)Hvec\(resid=\).*Newton'):
        prob.Hvec(None, v, resid=r)
    with pytest.raises(ValueError, match="'operator' or 'full'"):
        prob.Hvec(None, v, linearisation='scaler')
    with pytest.raises(ValueError, match='weights are real'):
        prob.Hvec(None, v, weights=-np.ones(sv.nD))
    # what the key does not open
    with pytest.raises(NotImplementedError, match=r'(?s)hessianBlocks.*Hvec\(parameter=\'joint\'\)'):
        prob.hessianBlocks(None)
    for kw in (dict(kind='gaussNewton'), dict(linearisation='operator'), dict(parameter='rho')):
        with pytest.raises(NotImplementedError, match="'scaler'"):
            prob.illumination(None, **kw)
    with pytest.raises(NotImplementedError, match='JvecBorn'):
        prob.Jvec(None, v)
    sc = dict(prob.systemConfig)
    p64 = za.Helm3DProblem(dict(sc, fieldsDtype='complex64'))
    p64.pair(za.Helm3DSurvey(sc))
    for par in ('c', 'rho', 'joint'):
        with pytest.raises(NotImplementedError, match='complex128'):
            p64.Jtvec(None, r, parameter=par, **X)
    with pytest.raises(ValueError, match='ky'):
        prob.fields(None, perKy=True)
    with pytest.raises(ValueError, match='one grid'):
        prob.fields(None, ownGrid=True)
    for wrapper in (za.MultiGridMultiFreq, za.ViscoMultiFreq, za.ViscoMultiGridMultiFreq):
        with pytest.raises(NotImplementedError, match='MultiFreq'):
            za.Helm3DProblem(dict(sc, SystemWrapper=wrapper))
