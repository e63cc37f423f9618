"""CPU: the multiscale family's geometry and host logic.  helm_regrid_axis (host only) against scipy's not-a-knot cubic interpolation;
MultiGridHelper scales and grids; the multigrid survey's per-scale vectors; the multiscale problem's host paths with the CPU oracle
for the solves and a scipy interpolator (the GridInterpolator key) for the transfers."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.interpolate import make_interp_spline, RectBivariateSpline

from zephyr_amd.interpolation import SplineGridInterpolator, regrid_axis
from zephyr_amd.distributors import MultiGridHelper, MultiGridMultiFreq
from zephyr_amd.survey import Helm2DMultiGridSurvey, HelmMultiGridSurvey
from zephyr_amd.problem import Helm2DProblem


def dense_axis(n_in, h_in, n_out, h_out):
    start, taps = regrid_axis(n_in, h_in, n_out, h_out)
    M = np.zeros((n_out, n_in))
    for j in range(n_out):
        M[j, start[j]:start[j] + taps.shape[1]] = taps[j]
    assert taps.shape[1] <= 64
    assert (start >= 0).all() and (start + taps.shape[1] <= n_in).all()
    return M


def scipy_axis(n_in, h_in, n_out, h_out):
    x = np.arange(n_in) * h_in
    p = np.clip(np.arange(n_out) * h_out, x[0], x[-1])
    return make_interp_spline(x, np.eye(n_in), k=3)(p)


@pytest.mark.parametrize('n_in,n_out,h_out', [
    (4, 9, 0.4), (5, 3, 2.), (57, 20, 2.9), (57, 57, 1.), (1024, 468, 1024 / 468.), (468, 1024, 468 / 1024.), (1024, 102, 1024 / 102.),
    (100, 10, 10.), (10, 100, 0.1), (101, 34, 3.), (34, 101, 1 / 3.),
    (57, 21, 2.9), (57, 19, 2.9),              # coarse grid beyond the fine extent (clamped) and short of it
    (1024, 747, 1.37),
])
def test_axis_matches_not_a_knot_spline(helm_lib, n_in, n_out, h_out):
    M = dense_axis(n_in, 1., n_out, h_out)
    R = scipy_axis(n_in, 1., n_out, h_out)
    assert np.abs(M - R).max() <= 1e-14


def test_axis_spacing_is_relative(helm_lib):
    assert np.abs(dense_axis(60, 9., 25, 9. * 2.4) - scipy_axis(60, 9., 25, 9. * 2.4)).max() <= 1e-14


def test_axis_rejects_short_grids(helm_lib):
    from zephyr_amd import _lib
    assert helm_lib.helm_regrid_axis(3, 1., 5, 0.5, None, None, 0) < 0
    with pytest.raises(_lib.HelmError):
        regrid_axis(3, 1., 5, .5)


@pytest.mark.parametrize('shape_a,shape_b,h', [((40, 57), (17, 23), 2.47), ((17, 23), (40, 57), 1 / 2.47), ((64, 48), (64, 48), 1.)])
def test_tensor_product_matches_rect_bivariate_spline(helm_lib, shape_a, shape_b, h):
    rng = np.random.default_rng(3)
    f = rng.standard_normal(shape_a)
    Wz = dense_axis(shape_a[0], 1., shape_b[0], h)
    Wx = dense_axis(shape_a[1], 1., shape_b[1], h)
    za, xa = np.arange(shape_a[0]), np.arange(shape_a[1])
    zb = np.clip(np.arange(shape_b[0]) * h, 0, za[-1])
    xb = np.clip(np.arange(shape_b[1]) * h, 0, xa[-1])
    ref = RectBivariateSpline(za, xa, f, kx=3, ky=3, s=0)(zb, xb, grid=True)
    assert np.abs(Wz @ f @ Wx.T - ref).max() <= 1e-14 * np.abs(ref).max() * 10


def base_config(**extra):
    sc = dict(nx=101, nz=80, dx=9., dz=9., freqs=[2., 5., 9.5], cMin=1500., targetGPW=8.)
    sc.update(extra)
    return sc


def test_helper_scales_clamp_and_complex_cmin():
    h = MultiGridHelper(base_config(freqs=[1., 2., 9.5, 40.]))
    expect = [min(max(1500. / f / 9. / 8., 1.), 10.) for f in (1., 2., 9.5, 40.)]
    assert np.allclose(h.scales, expect, rtol=0, atol=1e-15)
    assert h.scales[0] == 10. and h.scales[-1] == 1.
    hc = MultiGridHelper(base_config(cMin=1500. + 30j))
    assert np.allclose(hc.scales, [min(1500. / f / 9. / 8., 10.) for f in (2., 5., 9.5)])
    assert MultiGridHelper(base_config(freqs=[2., 20.], maxScale=4., minScale=2.)).scales == [4., 2.]


def test_scaled_grid_sizes_round_half_even():
    for nx, scale, snx in ((101, 2., 50), (103, 2., 52), (1024, 1024 / 468., 468), (30, 4., 8), (1024, 1500. / 2. / 9. / 8., 98)):
        ds = SplineGridInterpolator(dict(nx=nx, nz=20, dx=9., dz=9., scale=scale))
        assert ds.snx == snx == int(np.round(nx / scale))
        assert ds.sdx == 9. * scale
        assert ds.scaleUpdate == {'nx': snx, 'nz': int(np.round(20 / scale)), 'dx': 9. * scale, 'dz': 9. * scale}
        assert ds.shape == (snx * int(np.round(20 / scale)), nx * 20)
        assert ds.compression == scale ** 2


def test_upscaler_lands_on_native_grid():
    ds = SplineGridInterpolator(dict(nx=101, nz=101, dx=5., dz=5., scale=3.))
    assert (ds.snx, ds.snz) == (34, 34)
    up = ds.T
    assert int(np.round(34 * 3.)) == 102                          # (what the reference's transpose would make)
    assert (up.snx, up.snz, up.sdx, up.sdz) == (101, 101, 5., 5.)
    assert up.shape == (101 * 101, 34 * 34) and up.T is ds
    assert up.compression == pytest.approx(1 / 9.)


def test_helper_shares_interpolators_per_scale():
    h = MultiGridHelper(base_config(freqs=[2., 2., 40.]))
    ds = h.downScalers
    assert ds[0] is ds[1] and ds[2].identity
    assert [u.shape for u in h.upScalers] == [(d.shape[1], d.shape[0]) for d in ds]


def survey_config(mode='fixed', **extra):
    src = np.array([[100., 90.], [400., 120.], [700., 150.]])
    rec = np.stack([np.linspace(50., 850., 12), np.full(12, 600.)], axis=1)
    if mode == 'relative':
        rec = rec - src[0]
    sc = base_config(geom=dict(src=src, rec=rec, mode=mode))
    sc.update(extra)
    return sc


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_survey_vectors_on_each_scaled_grid(helm_lib, mode):
    sv = Helm2DMultiGridSurvey(survey_config(mode))
    helper = sv.mgHelper
    for ifreq in range(sv.nfreq):
        n = helper.downScalers[ifreq].shape[0]
        assert sv.sVecs(ifreq).shape == (n, sv.nsrc)
        for isrc in range(sv.nsrc):
            R = sv.rVec(isrc, ifreq)
            assert R.shape == (sv.nrec, n)
            assert sv.rVec(isrc, ifreq) is R                            # cached per scale (and source, in relative mode)
        if mode == 'relative':
            assert sv.rVec(0, ifreq) is not sv.rVec(1, ifreq)
            assert abs(sv.rVec(0, ifreq) - sv.rVec(1, ifreq)).sum() > 0
    assert sv.preProcessors is helper.downScalers and sv.postProcessors is helper.upScalers
    q = sv.getSources()
    assert [m.shape for m in q] == [(d.shape[0], sv.nsrc) for d in helper.downScalers]
    qb = sv.getResidualSources(np.ones((sv.nrec, sv.nsrc, sv.nfreq), dtype=np.complex128))
    assert [m.shape for m in qb] == [m.shape for m in q]


def test_single_grid_survey_ignores_frequency(helm_lib):
    from zephyr_amd.survey import Helm2DSurvey
    sv = Helm2DSurvey(survey_config())
    assert sv.sVecs(2) is sv.sVecs() and sv.rVec(0, 1) is sv.rVec(0)
    assert not isinstance(sv, HelmMultiGridSurvey)


# ---- host paths of a multiscale problem, solved by the CPU oracle ---------------------------------------------------------------------
class ScipyGridInterpolator(SplineGridInterpolator):
    'the reference\'s arithmetic (RectBivariateSpline on the reference\'s grids, target grid as SplineGridInterpolator)'

    def __mul__(self, rhs):
        if self.identity:
            return rhs
        rhs = np.asarray(rhs.toarray() if hasattr(rhs, 'toarray') else rhs)
        if rhs.ndim == 2:
            return np.stack([self * rhs[:, i] for i in range(rhs.shape[1])], axis=1)
        if np.iscomplexobj(rhs):
            return (self * rhs.real) + 1j * (self * rhs.imag)
        f = RectBivariateSpline(self.Z, self.X, rhs.reshape((self.nz, self.nx)), kx=3, ky=3, s=0)(self.sZ, self.sX, grid=True)
        return (f * self.gain).ravel()


def oracle_problem(**extra):
    from tests.doubles import OracleMiniZephyrHD
    rng = np.random.default_rng(5)
    nz, nx = 40, 48
    c = 2000. + 300. * rng.random((nz, nx))
    src = np.array([[100., 60.], [250., 80.]])
    rec = np.stack([np.linspace(40., 380., 7), np.full(7, 300.)], axis=1)
    sc = dict(nx=nx, nz=nz, dx=9., dz=9., c=c, rho=1000. + 200. * rng.random((nz, nx)), nPML=5, freqs=[6., 25.], cMin=1500., targetGPW=12.,
              Disc=OracleMiniZephyrHD, parallel=False, SystemWrapper=MultiGridMultiFreq, GridInterpolator=ScipyGridInterpolator,
              geom=dict(src=src, rec=rec, mode='fixed'), hostGradient=True)
    sc.update(extra)
    prob, sv = Helm2DProblem(sc), Helm2DMultiGridSurvey(sc)
    prob.pair(sv)
    return prob, sv, sc


def test_multiscale_problem_host_paths(helm_lib):
    prob, sv, sc = oracle_problem()
    scales = sv.mgHelper.scales
    assert scales[0] > 1. and scales[1] == 1.
    subs = prob.system.subProblems
    ds0 = sv.preProcessors[0]
    assert (subs[0].nz, subs[0].nx) == (ds0.snz, ds0.snx) and subs[0].dx == ds0.sdx
    assert np.allclose(np.ravel(subs[0].rho), ds0 * sc['rho'].ravel())             # rho on the coarse grid too (deviation 2)
    assert np.array_equal(np.ravel(subs[1].c), np.ravel(sc['c']).astype(np.complex128))
    u = prob.fields()
    assert [x.shape for x in u] == [(40 * 48, 2)] * 2
    d = sv.dpred()
    d_u = sv.dpred(u=u)                                   # (native-grid fields are brought back to the frequency's grid: up and down again)
    assert d_u.shape == d.shape and np.linalg.norm(d_u - d) <= 1e-2 * np.linalg.norm(d)
    resid = np.random.default_rng(1).standard_normal(d.shape) + 0j
    g = prob.Jtvec(v=resid)
    qf, qb = sv.getSources(), sv.getResidualSources(resid.reshape((sv.nrec, sv.nsrc, sv.nfreq)))
    ref = np.zeros(40 * 48, dtype=np.complex128)
    for i, sub in enumerate(subs):
        uM = sub * sp.hstack((qf[i], qb[i])).toarray()
        c = np.ravel(sub.c)
        om = 2 * np.pi * sv.freqs[i]
        pp = sv.postProcessors[i]
        ref += (pp * (-(om ** 2) / c ** 3)) * (pp * (uM[:, :2] * uM[:, 2:]).sum(axis=1))
    assert np.linalg.norm(g - ref) <= 1e-10 * np.linalg.norm(ref)
    g_u = prob.Jtvec(v=resid, u=u)
    assert g_u.shape == (40 * 48,) and np.isrealobj(g_u)
    dp = prob.Jvec(v=np.ones(40 * 48) * 1e-3)
    assert dp.shape == d.shape
