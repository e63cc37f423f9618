"""CPU: the 3-D survey layer without a GPU -- grid geometry and sources with `ny`, and the host maps of Helm3DProblem on an splu-backed stand-in for Helm3D
built on the oracle's matrix (tests/survey3d_cases.py): Taylor remainders of dpred, the adjoint identity through A^-T, what the forward factors give in
their place, and every refusal."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.special import i0

import zephyr_amd as za
from zephyr_amd import frechet3d
from zephyr_amd.base import BaseModelDependent
from zephyr_amd.problem import Helm2DProblem
from zephyr_amd.source import SimpleSource, SparseKaiserSource, KaiserSource, StackedSimpleSource, AnisotropicKaiserSource
from zephyr_amd.survey import Helm2DSurvey
from tests import survey3d_cases as s3

GRID = dict(nx=7, ny=6, nz=5, dx=10., dy=12., dz=8., xorig=3., yorig=-5., zorig=1.)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------
def test_linear_and_vector_indices_round_trip_in_3d():
    g = BaseModelDependent(GRID)
    assert g.modelDims == (5, 6, 7) and g.nrow == 210
    lin = np.arange(210)
    vec = g.toVecIndex(lin)
    assert vec.shape == (210, 3)
    assert np.array_equal(g.toLinearIndex(vec), lin)
    iz, iy, ix = np.unravel_index(lin, (5, 6, 7))
    assert np.array_equal(vec, np.stack([iz, iy, ix], axis=1))
    assert g.dy == 12. and g.yorig == -5.
    d = BaseModelDependent(dict(nx=7, ny=6, nz=5, dx=10.))
    assert d.dy == 10. and d.yorig == 0. and d.dz == 10.


def test_2d_geometry_and_sources_are_what_they_were():
    cfg = dict(nx=20, nz=24, dx=10., dz=8., xorig=2., zorig=-3.)
    g = BaseModelDependent(cfg)
    assert g.modelDims == (24, 20) and g.nrow == 480
    vec = np.array([[3, 4], [23, 19], [0, 0]])
    assert np.array_equal(g.toLinearIndex(vec), vec[:, 0] * 20 + vec[:, 1])
    assert np.array_equal(g.toVecIndex(np.array([64, 479, 0])), vec)
    locs = np.array([[57., 41.], [102., 77.], [2., -3.], [47., 9.]])            # (the last one: a tie in x between two nodes)
    s = SimpleSource(cfg)
    z, x = np.mgrid[-3.:-3. + 8. * 24:8., 2.:2. + 10. * 20:10.]
    want = np.array([np.argmin(np.sqrt((x - lx) ** 2 + (z - lz) ** 2).ravel()) for lx, lz in locs])
    assert np.array_equal(s.linIndexOf(locs), want)
    q = s(locs)
    assert q.shape == (480, 4) and np.array_equal(np.flatnonzero(q[:, 0]), want[:1])
    k = SparseKaiserSource(cfg)
    col = np.asarray(k(locs[:1]).todense()).reshape((24, 20))
    Zi, Xi = want[0] // 20, want[0] % 20
    patch = (1. / (10. * 8.)) * k.kws((locs[0, 0] - 2. - Xi * 10., locs[0, 1] + 3. - Zi * 8.), Zi, Xi)
    ref = np.zeros((24, 20), dtype=np.complex128)
    ref[Zi - 4:Zi + 5, Xi - 4:Xi + 5] = patch
    assert np.array_equal(col, ref)                                             # the same bits: the 2-D path is the unchanged code


# ---- sources --------------------------------------------------------------------------------------------------------------------------------------
def test_simple_source_nearest_node_on_node_off_node_and_tie():
    s = SimpleSource(GRID)
    node = lambda iz, iy, ix: (iz * 6 + iy) * 7 + ix
    on = [3. + 10. * 4, -5. + 12. * 2, 1. + 8. * 3]
    off = [3. + 10. * 4 + 4.9, -5. + 12. * 2 - 5.9, 1. + 8. * 3 + 3.9]
    tie = [3. + 10. * 4 + 5., -5. + 12. * 2 + 6., 1. + 8. * 3 + 4.]               # half-way on every axis: the first minimum, as np.argmin
    far = [-100., 1000., 1. + 8. * 1]
    got = s.linIndexOf(np.array([on, off, tie, far]))
    assert list(got) == [node(3, 2, 4), node(3, 2, 4), node(3, 2, 4), node(1, 5, 0)]
    # the same answer as the full distance field's argmin, built here
    z, y, x = np.mgrid[0:5, 0:6, 0:7]
    for loc, g in zip([on, off, far], got[[0, 1, 3]]):
        d2 = (3. + 10. * x - loc[0]) ** 2 + (-5. + 12. * y - loc[1]) ** 2 + (1. + 8. * z - loc[2]) ** 2
        assert np.argmin(d2.ravel()) == g
    assert np.array_equal(s.vecIndexOf(np.array([on])), [[3, 2, 4]])
    q = s(np.array([on, far]))
    assert q.shape == (210, 2) and q.dtype == np.complex128
    assert np.array_equal(np.argwhere(q), [[node(1, 5, 0), 1], [node(3, 2, 4), 0]]) and q.sum() == 2.
    with pytest.raises(ValueError, match='triples'):
        s.linIndexOf(np.array([[1., 2.]]))


HC4 = 6.31


def response1(off, ireg=4, b=HC4):
    'the 1-D Kaiser-windowed sinc of Hicks (2002) at the 2 ireg + 1 nodes around the nearest one, written here independently of the product code'
    out = np.zeros(2 * ireg + 1)
    for j in range(-ireg, ireg + 1):
        d = off - j                                   # distance (in cells) of the source from node j of the patch
        w = i0(b * np.sqrt(max(0., 1. - (d / ireg) ** 2))) / i0(b)     # (beyond the half-width the window stays at its edge value 1 / I0(b), as in 2-D)
        out[j + ireg] = np.sinc(d) * w
    return out


def expected_column(cfg, loc, ireg=4):
    nz, ny, nx = cfg['nz'], cfg['ny'], cfg['nx']
    axes = ((cfg['xorig'], cfg['dx'], nx), (cfg['yorig'], cfg['dy'], ny), (cfg['zorig'], cfg['dz'], nz))
    vec = []
    for a, (o, d, n) in enumerate(axes):
        node = int(np.argmin(np.abs(o + d * np.arange(n) - loc[a])))
        r = response1(loc[a] - o - node * d, ireg)                    # (the offset as the 2-D generator takes it, source.py:213-230)
        full = np.zeros(n)
        for j in range(-ireg, ireg + 1):
            if 0 <= node + j < n:
                full[node + j] = r[j + ireg]
        vec.append(full)
    vx, vy, vz = vec
    return (vz[:, None, None] * vy[None, :, None] * vx[None, None, :]) / (cfg['dx'] * cfg['dy'] * cfg['dz'])


KCFG = dict(nx=22, ny=19, nz=20, dx=1., dy=1., dz=1., xorig=0., yorig=0., zorig=0.)


@pytest.mark.parametrize('loc', [
    (10.3, 9.6, 10.2),                     # centred: the whole 9^3 patch
    (1.3, 9.6, 10.2), (20.4, 9.6, 10.2),   # clipped at the two x faces
    (10.3, 0.8, 10.2), (10.3, 17.1, 10.2), # the two y faces
    (10.3, 9.6, 2.2), (10.3, 9.6, 18.7),   # the two z faces
    (0.4, 17.8, 0.3),                      # a corner
], ids=['centre', 'x-', 'x+', 'y-', 'y+', 'z-', 'z+', 'corner'])
def test_sparse_kaiser_source_is_the_separable_product(loc):
    k = SparseKaiserSource(KCFG)
    q = k(np.array([loc]))
    assert sp.issparse(q) and q.shape == (22 * 19 * 20, 1)
    got = np.asarray(q.todense()).reshape((20, 19, 22))
    want = expected_column(KCFG, loc)
    # the two codes form the node distance differently (off + ireg - i against off - j): it differs by up to 2 ulp(8) = 1.8e-15, sinc and the window have
    # slopes below 1.4 and 2 there, every factor is at most 1 in magnitude -- 3 factors x (1.4 + 2) x 1.8e-15 plus a few relative ulps, under 2e-14 absolute
    assert np.abs(got - want).max() <= 2e-14
    assert np.count_nonzero(got) <= 729 and (np.count_nonzero(got) == 729) == (loc == (10.3, 9.6, 10.2))
    assert np.array_equal(KaiserSource(KCFG)(np.array([loc])), q.toarray())


def test_sparse_kaiser_source_scaling_delta_and_free_surface():
    cfg = dict(KCFG, dx=10., dy=12., dz=8.)
    on = np.array([[100., 108., 80.]])                       # an interior node
    q = SparseKaiserSource(cfg)(on)
    assert abs(q.sum() - 1. / 960.) <= 1e-15 / 960.          # sinc vanishes at the other nodes: the column is the scaled delta
    q0 = SparseKaiserSource(dict(cfg, ireg=0))(np.array([[103., 104., 83.], [0., 0., 0.]]))
    assert q0.nnz == 2 and np.array_equal(q0.tocoo().row[np.argsort(q0.tocoo().col)], [(10 * 19 + 9) * 22 + 10, 0]) and np.all(q0.data == 1. / 960.)
    with pytest.raises(ValueError, match='free surface'):
        SparseKaiserSource(dict(cfg, freeSurf=(True, False, False, False)))(on)
    for cls in (StackedSimpleSource, AnisotropicKaiserSource):
        with pytest.raises(NotImplementedError, match='3-D'):
            cls(cfg)


# ---- the host maps on the oracle ---------------------------------------------------------------------------------------------------------------------
_PAIRS = {}


def pair(grid, mode='fixed'):
    'one problem / survey pair per case for the whole module: the LU factors of the base model are made once'
    if (grid, mode) not in _PAIRS:
        prob, sv = s3.host_pair(grid, mode)
        _PAIRS[(grid, mode)] = (prob, sv, np.array(prob.systemConfig['c']))
    return _PAIRS[(grid, mode)]


def test_mass_stencil_is_the_model_derivative_of_the_oracle_matrix():
    "d A / d c along dc from two oracle matrices against M~ diag(chi dc): the formula the routes are built on, boundary nodes included"
    prob, sv, c0 = pair('12x11x13')
    op = prob.system.subProblems[0]
    rng = np.random.default_rng(4)
    dc = rng.standard_normal(c0.shape)
    h = 1e-3
    base = dict(prob.systemConfig, freq=sv.freqs[0])
    Ap = s3.oracle_matrix(s3.OracleHelm3D(dict(base, c=c0 + h * dc)))
    Am = s3.oracle_matrix(s3.OracleHelm3D(dict(base, c=c0 - h * dc)))
    dA = (Ap - Am) / (2 * h)
    M = frechet3d.massStencil3(op.modelDims)
    want = M @ sp.diags(frechet3d.velocityChain3(op) * dc.ravel())
    assert abs(dA - want).max() <= 1e-6 * abs(want).max()               # (central difference: O(h^2 / c^2))
    assert M.shape == (op.nrow, op.nrow) and abs(M - M.T).max() > 0.01   # symmetric weights, but the boundary rows are masked: M~ != M~^T
    inside = frechet3d.interiorMask3(op.modelDims)
    assert np.all(np.diff(M.indptr)[inside] == 27) and np.all(np.diff(M.indptr)[~inside] == 0)
    assert np.allclose(M.sum(axis=1).A1[inside], 1.0, rtol=0, atol=1e-15)


@pytest.mark.parametrize('grid,mode', [('12x11x13', 'fixed'), ('12x11x13', 'relative'), ('18x16x20', 'fixed')])
def test_taylor_remainders_of_dpred_fall_fourfold(grid, mode):
    prob, sv, c0 = pair(grid, mode)
    rng = np.random.default_rng(7)
    dc = 40. * rng.uniform(-1., 1., c0.shape)
    d0 = sv.dpred(c0)
    J = prob.JvecBorn(c0, dc.ravel(), linearisation='operator')
    assert np.array_equal(J, prob.JvecBorn(c0, dc.ravel(), linearisation='full'))         # the same derivative, the same arrays
    F = prob.fields(c0)
    assert s3.rel(prob.JvecBorn(c0, dc.ravel(), u=F, linearisation='operator'), J) <= 1e-13
    rem = []
    for j in range(6):
        h = 0.5 ** j
        rem.append(np.linalg.norm(sv.dpred(c0 + h * dc) - d0 - h * J))
    prob.updateModel(c0)
    ratios = [rem[j] / rem[j + 1] for j in range(5)]
    print('%s %s: Taylor remainders %s, ratios %s' % (grid, mode, ['%.3e' % r for r in rem], ['%.3f' % r for r in ratios]))
    assert all(3.9 <= r <= 4.1 for r in ratios), ratios
    assert rem[0] > 1e-3 * np.linalg.norm(J)                             # (the step is not in the linear regime by accident: the remainder is visible)


@pytest.mark.parametrize('grid,mode', [('12x11x13', 'fixed'), ('12x11x13', 'relative'), ('18x16x20', 'fixed')])
def test_adjoint_identity_through_the_transposed_factors(grid, mode):
    prob, sv, c0 = pair(grid, mode)
    rng = np.random.default_rng(8)
    v = rng.standard_normal(prob.nrow)
    r = s3.randc(rng, sv.nD)
    Jv = prob.JvecBorn(c0, v, linearisation='operator')
    g = prob.Jtvec(c0, r, adjoint='transpose', linearisation='operator')
    assert g.dtype == np.float64 and g.shape == (prob.nrow,)
    assert np.array_equal(g, prob.Jtvec(c0, r, adjoint='transpose', linearisation='full'))
    lhs, rhs = s3.inner(r, Jv), float(g @ v)
    miss = abs(lhs - rhs) / abs(lhs)
    print('%s %s: adjoint identity misses by %.2e' % (grid, mode, miss))
    assert miss <= 1e-12
    F = prob.fields(c0)
    assert s3.rel(prob.Jtvec(c0, r, u=F, adjoint='transpose', linearisation='operator'), g) <= 1e-12
    assert all(sub.transposed for sub in prob.adjointSystem.subProblems) and not any(sub.transposed for sub in prob.system.subProblems)
    # the same expression with the FORWARD factors in the place of the transposed ones is not the adjoint
    keep = prob._adjointSystem
    try:
        prob._adjointSystem = prob.system
        gw = prob.Jtvec(c0, r, adjoint='transpose', linearisation='operator')
    finally:
        prob._adjointSystem = keep
    wrong = abs(lhs - float(gw @ v)) / abs(lhs)
    print('%s %s: with the forward factors the identity misses by %.2f; the gradients differ by %.2f of the norm' % (grid, mode, wrong, s3.rel(gw, g)))
    assert wrong > 0.1


def test_boundary_nodes_count_as_columns():
    prob, sv, c0 = pair('12x11x13')
    dc = np.zeros(c0.shape)
    dc[0], dc[-1], dc[:, 0], dc[:, -1], dc[:, :, 0], dc[:, :, -1] = 1., 1., 1., 1., 1., 1.
    J = prob.JvecBorn(c0, dc.ravel(), linearisation='operator')
    assert np.linalg.norm(J) > 0
    # u^ on a boundary node is premul q there (an identity row), so only the source whose patch reaches the faces contributes, and little: the data move by
    # 1e-9 of their size per m/s.  That is still far above rounding, and it is the derivative: a finite step reproduces it
    d0 = sv.dpred(c0)
    diff = sv.dpred(c0 + 50. * dc) - d0
    prob.updateModel(c0)
    print('boundary nodes: |J| = %.3e, |d0| = %.3e, finite step against 50 J: %.2e' % (np.linalg.norm(J), np.linalg.norm(d0), s3.rel(diff, 50. * J)))
    assert s3.rel(diff, 50. * J) <= 0.1            # (c changes by 2.5 % on those nodes: the remainder is of that order, not of order 1)
    g = prob.Jtvec(c0, s3.randc(np.random.default_rng(1), sv.nD), adjoint='transpose', linearisation='operator')
    assert np.abs(g.reshape(c0.shape)[0]).max() > 0                      # and they receive a gradient


def test_reference_gradient_and_scaler_routes_on_the_host():
    "the reference's form: sum_f gradientScaler (.) sum_s uF (.) uB through the forward factors (mux: complex; u given: its real part)"
    prob, sv, c0 = pair('12x11x13')
    r = s3.randc(np.random.default_rng(3), sv.nD)
    F = prob.fields(c0)
    qb = sv.getResidualSources(r.reshape((sv.nrec, sv.nsrc, sv.nfreq)))
    st = complex(prob.system.scaleTerm)
    want = sum(prob.gradientScaler(i) * (F[i] * (st * (prob.system.subProblems[i] * qb[i]))).sum(axis=1) for i in range(sv.nfreq))
    g = prob.Jtvec(c0, r)
    assert g.dtype == np.complex128 and s3.rel(g, want) <= 1e-12
    assert s3.rel(prob.Jtvec(c0, r, u=F), want.real) <= 1e-12
    assert s3.rel(sv.dpred(c0, u=F), sv.dpred(c0)) <= 1e-14
    gt = prob.Jtvec(c0, r, u=F, adjoint='transpose')                      # 'scaler' through A^-T: the exact adjoint of the 'scaler' Born data
    v = np.random.default_rng(5).standard_normal(prob.nrow)
    assert abs(s3.inner(r, prob.JvecBorn(c0, v, u=F)) - float(gt @ v)) <= 1e-12 * abs(float(gt @ v))
    H = prob.illumination(c0, u=F, kind='energy')
    assert s3.rel(H, sum((np.abs(f) ** 2).sum(axis=1) for f in F)) <= 1e-14
    del prob.factors


def test_refusals_name_the_remedy():
    prob, sv, c0 = pair('12x11x13')
    r, v = np.zeros(sv.nD, dtype=complex), np.zeros(prob.nrow)
    sc = dict(prob.systemConfig)
    norho = dict(sc)
    del norho['rho']
    p2, s2 = za.Helm3DProblem(norho), za.Helm3DSurvey(norho)
    p2.pair(s2)
    for call in (lambda: p2.Jtvec(c0, r, adjoint='transpose', linearisation='operator'), lambda: p2.JvecBorn(c0, v, linearisation='full')):
        with pytest.raises(NotImplementedError, match=r'(?s)rho.*Gardner.*Laplacian'):
            call()
    for par in ('rho', 'joint', 'Q'):
        with pytest.raises(NotImplementedError, match="parameter='c'"):
            prob.Jtvec(c0, r, adjoint='transpose', linearisation='operator', parameter=par)
        with pytest.raises(NotImplementedError, match="parameter='c'"):
            prob.JvecBorn(c0, v, linearisation='operator', parameter=par)
    with pytest.raises(ValueError, match="adjoint='transpose'"):
        prob.Jtvec(c0, r, linearisation='operator')
    with pytest.raises(NotImplementedError, match='JvecBorn'):
        prob.Jvec(c0, v)
    with pytest.raises(NotImplementedError, match='Jtvec'):
        prob.Hvec(c0, v)
    with pytest.raises(NotImplementedError, match='illumination'):
        prob.hessianBlocks(c0)
    for kw in (dict(kind='gaussNewton'), dict(linearisation='operator'), dict(linearisation='full')):
        with pytest.raises(NotImplementedError, match="'scaler'"):
            prob.illumination(c0, **kw)
    p64 = za.Helm3DProblem(dict(sc, fieldsDtype='complex64'))
    p64.pair(za.Helm3DSurvey(sc))
    with pytest.raises(NotImplementedError, match='complex128'):
        p64.Jtvec(c0, r, adjoint='transpose', linearisation='operator')
    with pytest.raises(ValueError, match='ky'):
        prob.fields(c0, perKy=True)
    with pytest.raises(ValueError, match='one grid'):
        prob.fields(c0, ownGrid=True)
    with pytest.raises(ValueError, match='ky'):
        prob.fieldsDevice(c0, perKy=True)
    for wrapper in (za.MultiGridMultiFreq, za.ViscoMultiFreq, za.ViscoMultiGridMultiFreq):
        with pytest.raises(NotImplementedError, match='MultiFreq'):
            za.Helm3DProblem(dict(sc, SystemWrapper=wrapper))
    # a 2-D survey with a 3-D problem and the other way round
    sc2 = {k: val for k, val in sc.items() if k not in ('ny', 'dy')}
    sc2.update(c=2000., rho=1000., geom=dict(src=np.array([[50., 50.]]), rec=np.array([[60., 60.]])), Disc=za.MiniZephyr)
    with pytest.raises(TypeError, match='Helm3DSurvey'):
        prob.pair(Helm2DSurvey(sc2))
    with pytest.raises(TypeError, match='Helm2DSurvey'):
        Helm2DProblem(sc2).pair(sv)
    with pytest.raises(ValueError, match='ny'):
        za.Helm3DProblem(sc2)
    with pytest.raises(ValueError, match='ny'):
        za.Helm3DSurvey(sc2)
    with pytest.raises(ValueError, match=r'\(x, y, z\)'):
        za.Helm3DSurvey(dict(sc, geom=dict(src=np.array([[50., 50.]]), rec=np.array([[60., 60., 1.]]))))


def test_transposed_class_and_plane_formula():
    sc = dict(s3.survey_config((12, 11, 13), 3, (5., 6.), 'fixed'), freq=5.)
    assert za.Helm3D.Transposed is za.Helm3DTransposed and za.Helm3DTransposed(sc).transposed is True and za.Helm3D(sc).transposed is False
    with pytest.raises(NotImplementedError):
        za.Helm3D(dict(sc, transposed=True))                   # (the key stays refused: the transposed operator is a class)
    A, AT = s3.OracleHelm3D(sc).A, s3.OracleHelm3DT(sc).A
    offd = A - sp.diags(A.diagonal())
    assert abs(A.T - AT).max() == 0 and abs(A - AT).max() > 0.1 * abs(offd).max()         # and A is far from symmetric on the scale of its couplings
    # the planes of the transpose by the formula the kernel implements
    from oracle import helm3d_oracle as h3
    C = h3.helm3d_coefficients(12, 11, 13, sc['c'], sc['rho'], 5., dx=10., dy=9., dz=11., nPML=3, cPML=250.)
    assert abs(h3.coefficients_to_csr3(s3.transpose_planes3(C)) - h3.coefficients_to_csr3(C).T).max() == 0
