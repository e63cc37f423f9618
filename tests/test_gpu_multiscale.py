"""GPU: the multiscale family.  helm_regrid_apply[_device] against scipy's RectBivariateSpline; MultiGridMultiFreq against single-grid
sub-problems configured by hand on the scipy-resampled model; the multiscale survey / problem pair on its device and host paths."""
import os
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.interpolate import RectBivariateSpline

pytestmark = pytest.mark.gpu


def spline(f, src, dst):
    'scipy reference: field f on grid src = (nz, nx, dz, dx) evaluated on grid dst (same origin, points clamped)'
    nz, nx, dz, dx = src
    Z, X = dz * np.arange(nz), dx * np.arange(nx)
    zb, xb = np.clip(dst[2] * np.arange(dst[0]), 0, Z[-1]), np.clip(dst[3] * np.arange(dst[1]), 0, X[-1])
    f = np.asarray(f).reshape((nz, nx))
    if np.iscomplexobj(f):
        return spline(f.real, src, dst) + 1j * spline(f.imag, src, dst)
    return RectBivariateSpline(Z, X, f, kx=3, ky=3, s=0)(zb, xb, grid=True).ravel()


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


def fields(rng, n, k):
    return rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))


@pytest.mark.parametrize('scale', [2.37, 1 / 2.37, 3.])
def test_regrid_host_arrays_match_scipy(helm_lib, scale):
    from zephyr_amd.interpolation import SplineGridInterpolator
    ds = SplineGridInterpolator(dict(nx=83, nz=61, dx=9., dz=9., scale=scale, device=0))
    src, dst = (61, 83, 9., 9.), (ds.snz, ds.snx, ds.sdz, ds.sdx)
    rng = np.random.default_rng(1)
    f = fields(rng, 61 * 83, 5)
    out = ds * f
    assert out.shape == (ds.snz * ds.snx, 5)
    for j in range(5):
        assert rel(out[:, j], spline(f[:, j], src, dst)) <= 1e-13
    one = ds * f[:, 2].real                            # real (N,) in, real out
    assert one.dtype == np.float64 and rel(one, spline(f[:, 2].real, src, dst)) <= 1e-13
    e = SplineGridInterpolator(dict(nx=83, nz=61, dx=9., dz=9., scale=scale, eCons=True, device=0))
    assert rel(e * f[:, 0], scale ** 2 * spline(f[:, 0], src, dst)) <= 1e-13
    assert rel(e.T * (e * f[:, 0]), spline(spline(f[:, 0], src, dst), dst, src)) <= 1e-13      # eCons: scale^2 down, 1/scale^2 up


@pytest.mark.parametrize('layout', ['kN', 'Nk'])
def test_regrid_device_layouts_beta_mul(helm_lib, layout):
    import torch
    from zephyr_amd.interpolation import SplineGridInterpolator
    dev = torch.device('cuda', 0)
    ds = SplineGridInterpolator(dict(nx=96, nz=70, dx=10., dz=10., scale=2.6, device=0))
    for t in (ds, ds.T):
        na, nb = t.shape[1], t.shape[0]
        src, dst = (t.nz, t.nx, t.dz, t.dx), (t.snz, t.snx, t.sdz, t.sdx)
        rng = np.random.default_rng(7)
        k = 6
        f = fields(rng, na, k)
        prev = fields(rng, nb, k)
        mul = fields(rng, nb, 1)[:, 0]
        if layout == 'kN':
            dIn, dOut = torch.from_numpy(np.ascontiguousarray(f.T)).to(dev), torch.from_numpy(np.ascontiguousarray(prev.T)).to(dev)
        else:
            dIn, dOut = torch.from_numpy(f.copy()).to(dev), torch.from_numpy(prev.copy()).to(dev)
        dMul = torch.from_numpy(mul).to(dev)
        t.apply_device(dIn, dOut, k=k, gain=0.5 - 0.25j, beta=1., mul=dMul, layout=layout)
        got = dOut.cpu().numpy()
        got = got.T if layout == 'kN' else got
        for j in range(k):
            ref = prev[:, j] + mul * ((0.5 - 0.25j) * spline(f[:, j], src, dst))
            assert rel(got[:, j], ref) <= 1e-13


def test_regrid_job_size(helm_lib):
    'at the bench job\'s size: 256 fields 468^2 -> 1024^2 in the (k, N) layout; the host-array path computes the same bits'
    import torch
    from zephyr_amd.interpolation import SplineGridInterpolator
    dev = torch.device('cuda', 0)
    up = SplineGridInterpolator(dict(nx=1024, nz=1024, dx=9., dz=9., scale=1024 / 468., device=0)).T
    assert up.shape == (1024 * 1024, 468 * 468)
    k = 256
    g = torch.Generator(device=dev).manual_seed(3)
    dIn = torch.randn((k, 468 * 468), dtype=torch.complex128, device=dev, generator=g)
    dOut = torch.empty((k, 1024 * 1024), dtype=torch.complex128, device=dev)
    up.apply_device(dIn, dOut, k=k)
    pick = [0, 131, 255]
    fin = dIn[pick].cpu().numpy()
    got = dOut[pick].cpu().numpy()
    host = up * np.ascontiguousarray(fin.T)
    assert np.array_equal(host.T, got)
    src, dst = (468, 468, up.dz, up.dx), (1024, 1024, up.sdz, up.sdx)
    for j, f in enumerate(fin):
        assert rel(got[j], spline(f, src, dst)) <= 1e-13


# ---- MultiGridMultiFreq against hand-made single-grid sub-problems --------------------------------------------------------------------
def model(nz=72, nx=90, seed=2):
    rng = np.random.default_rng(seed)
    c = 1800. + 700. * rng.random((nz, nx))
    rho = 1000. + 500. * rng.random((nz, nx))
    return c, rho


def test_multigrid_multifreq_matches_hand_configured(helm_lib):
    from zephyr_amd import MiniZephyr, MultiFreq, MultiGridMultiFreq, SimpleSource
    c, rho = model()
    nz, nx = c.shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, rho=rho, nPML=8, freqs=[4., 30.], cMin=1800., targetGPW=10., Disc=MiniZephyr,
              parallel=False, device=0)
    mg = MultiGridMultiFreq(sc)
    ds = mg.mgHelper.downScalers
    assert ds[0].scale > 1 and ds[1].identity
    q = [SimpleSource(dict(sc, **d.scaleUpdate))(np.array([[300., 320.], [500., 200.]])) for d in ds]
    us = list(mg * q)
    # frequency 0 by hand: a single-grid MultiFreq on the scipy-resampled model
    d = ds[0]
    src, dst = (nz, nx, 10., 10.), (d.snz, d.snx, d.sdz, d.sdx)
    hand = dict(sc, nx=d.snx, nz=d.snz, dx=d.sdx, dz=d.sdz, c=spline(c, src, dst), rho=spline(rho, src, dst), freqs=[4.])
    for key in ('cMin', 'targetGPW'):
        hand.pop(key)
    ref = list(MultiFreq(hand) * q[0])[0]
    assert us[0].shape == ref.shape and rel(us[0], ref) <= 1e-10
    # frequency 1 has scale 1: the same bits as MultiFreq
    ref1 = list(MultiFreq(dict(sc, freqs=[30.])) * q[1])[0]
    assert np.array_equal(us[1], ref1)


def test_multigrid_eurus_tti_heterogeneous(helm_lib):
    from zephyr_amd import Eurus, MultiFreq, MultiGridMultiFreq, SimpleSource
    c, rho = model(64, 80, seed=4)
    nz, nx = c.shape
    rng = np.random.default_rng(9)
    theta = 0.4 * rng.random((nz, nx))
    eps = 0.1 * rng.random((nz, nx))
    delta = 0.05 * rng.random((nz, nx))
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, rho=rho, theta=theta, eps=eps, delta=delta, nPML=8, freqs=[5.], cMin=1800., targetGPW=12.,
              Disc=Eurus, parallel=False, device=0)
    mg = MultiGridMultiFreq(sc)
    d = mg.mgHelper.downScalers[0]
    assert d.scale > 1
    q = SimpleSource(dict(sc, **d.scaleUpdate))(np.array([[300., 320.]]))
    u = list(mg * [q])[0]
    src, dst = (nz, nx, 10., 10.), (d.snz, d.snx, d.sdz, d.sdx)
    hand = dict(sc, nx=d.snx, nz=d.snz, dx=d.sdx, dz=d.sdz, freqs=[5.], **{k: spline(v, src, dst) for k, v in
                                                                         dict(c=c, rho=rho, theta=theta, eps=eps, delta=delta).items()})
    ref = list(MultiFreq(hand) * q)[0]
    assert rel(u, ref) <= 1e-10


# ---- survey / problem pairing ----------------------------------------------------------------------------------------------------------
def pair(problem=None, survey=None, **extra):
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    c, rho = model(80, 96, seed=6)
    nz, nx = c.shape
    src = np.stack([np.linspace(150., 800., 5), np.full(5, 120.)], axis=1)
    rec = np.stack([np.linspace(100., 850., 16), np.full(16, 650.)], axis=1)
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=c, rho=rho, nPML=8, freqs=[3., 6., 30.], cMin=1800., targetGPW=10., Disc=MiniZephyr,
              SystemWrapper=MultiGridMultiFreq, geom=dict(src=src, rec=rec, mode='fixed'))
    sc.update(extra)
    prob = (problem or Helm2DProblem)(sc)
    sv = (survey or Helm2DMultiGridSurvey)(sc)
    prob.pair(sv)
    return prob, sv, sc


def host_gradient(prob, sv, resid):
    'mux gradient with scipy up-scaling: sum_f up(-(w^2/c_f^3)) (.) up(scale^2 sum_s uF (.) uB)'
    qf, qb = sv.getSources(), sv.getResidualSources(resid.reshape((sv.nrec, sv.nsrc, sv.nfreq)))
    g = np.zeros(prob.nrow, dtype=np.complex128)
    ns = sv.nsrc
    for i, sub in enumerate(prob.system.subProblems):
        u = sub * sp.hstack((qf[i], qb[i])).tocsc()
        cf = np.ravel(sub.c)
        om = 2 * np.pi * sv.freqs[i]
        src = (sub.nz, sub.nx, sub.dz, sub.dx)
        dst = (prob.nz, prob.nx, prob.dz, prob.dx)
        up = (lambda f: f) if src[:2] == dst[:2] else (lambda f: spline(f, src, dst))
        g += up(-(om ** 2) / cf ** 3) * up((u[:, :ns] * u[:, ns:]).sum(axis=1))
    return g


def test_dpred_and_jtvec_device_match_host(helm_lib):
    prob, sv, sc = pair()
    probh, svh, _ = pair(hostGradient=True)
    assert prob._deviceGradientAvailable() and not probh._deviceGradientAvailable()
    d = sv.dpred()
    dh = svh.dpred()
    assert rel(d, dh) <= 1e-12
    resid = np.random.default_rng(3).standard_normal(d.shape) + 1j * np.random.default_rng(4).standard_normal(d.shape)
    g = prob.Jtvec(v=resid)
    ref = host_gradient(prob, sv, resid)
    assert g.shape == (prob.nrow,) and rel(g, ref) <= 1e-10
    assert rel(probh.Jtvec(v=resid), ref) <= 1e-10


def test_fields_u_branch_and_jvec(helm_lib):
    prob, sv, sc = pair(hostGradient=True)
    u = prob.fields()
    assert [x.shape for x in u] == [(prob.nrow, sv.nsrc)] * sv.nfreq
    subs = prob.system.subProblems
    q = sv.getSources()
    for i in (0, 2):
        coarse = subs[i] * q[i]
        src, dst = (subs[i].nz, subs[i].nx, subs[i].dz, subs[i].dx), (prob.nz, prob.nx, prob.dz, prob.dx)
        ref = coarse if src[:2] == dst[:2] else np.stack([spline(coarse[:, j], src, dst) for j in range(sv.nsrc)], axis=1)
        assert rel(u[i], ref) <= 1e-12
    resid = np.random.default_rng(5).standard_normal(sv.nD) + 0j
    qb = sv.getResidualSources(resid.reshape((sv.nrec, sv.nsrc, sv.nfreq)))
    g = prob.Jtvec(v=resid, u=u)
    ref = np.zeros(prob.nrow, dtype=np.complex128)
    for i, sub in enumerate(subs):
        ub = sub * qb[i]
        src, dst = (sub.nz, sub.nx, sub.dz, sub.dx), (prob.nz, prob.nx, prob.dz, prob.dx)
        up = (lambda f: f) if src[:2] == dst[:2] else (lambda f: spline(f, src, dst))
        om = 2 * np.pi * sv.freqs[i]
        ubf = np.stack([up(ub[:, j]) for j in range(sv.nsrc)], axis=1)
        ref += up(-(om ** 2) / np.ravel(sub.c) ** 3) * (u[i] * ubf).sum(axis=1)
    assert np.isrealobj(g) and rel(g, ref.real) <= 1e-10
    v = np.random.default_rng(6).standard_normal(prob.nrow)
    dp = prob.Jvec(v=v)
    assert dp.shape == (sv.nD,) and np.all(np.isfinite(dp))
    i = 0
    sub = subs[i]
    om = 2 * np.pi * sv.freqs[i]
    src, dst = (sub.nz, sub.nx, sub.dz, sub.dx), (prob.nz, prob.nx, prob.dz, prob.dx)
    sens = spline(-(np.ravel(sub.c) ** 3) / om ** 2, src, dst)
    uv = sub * spline(v * sens, dst, src).reshape((-1, 1))
    ref0 = np.outer(sv.rVec(0, i) @ uv, q[i].T @ uv)
    assert rel(dp.reshape((sv.nrec, sv.nsrc, sv.nfreq))[:, :, i], ref0) <= 1e-10


def test_visco_multigrid_problem(helm_lib):
    from zephyr_amd.problem import Helm2DViscoMultiGridProblem
    from zephyr_amd import MiniZephyr
    c, _ = model(80, 96, seed=6)
    Q = 40. + 60. * np.random.default_rng(8).random(c.shape)
    from zephyr_amd import ViscoMultiGridMultiFreq
    prob, sv, sc = pair(problem=Helm2DViscoMultiGridProblem, Q=Q, freqBase=5., SystemWrapper=ViscoMultiGridMultiFreq)
    probh, svh, _ = pair(problem=Helm2DViscoMultiGridProblem, Q=Q, freqBase=5., SystemWrapper=ViscoMultiGridMultiFreq, hostGradient=True)
    subs = prob.system.subProblems
    d0 = sv.preProcessors[0]
    fact = 1. + np.log(3. / 5.) / (np.pi * Q)
    cR = fact * sc['c']
    cfine = (cR + 0.5j * cR / Q).ravel()
    src, dst = (prob.nz, prob.nx, prob.dz, prob.dx), (d0.snz, d0.snx, d0.sdz, d0.sdx)
    assert rel(np.ravel(subs[0].c), spline(cfine, src, dst)) <= 1e-13
    assert rel(prob.system.spUpdates[0]['Q'], spline(Q, src, dst)) <= 1e-13
    d = sv.dpred()
    assert rel(d, svh.dpred()) <= 1e-12
    resid = np.random.default_rng(2).standard_normal(d.shape) + 0j
    assert rel(prob.Jtvec(v=resid), host_gradient(prob, sv, resid)) <= 1e-10


def test_25d_multigrid_survey(helm_lib):
    from zephyr_amd import MiniZephyr25D
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DMultiGridSurvey
    prob, sv, sc = pair(problem=Helm25DProblem, survey=Helm25DMultiGridSurvey, Disc=MiniZephyr25D, nky=3, freqs=[3., 30.], parallel=False)
    assert not prob._deviceGradientAvailable()
    d = sv.dpred()
    assert d.shape == (sv.nD,) and np.all(np.isfinite(d)) and np.abs(d).max() > 0
    resid = np.random.default_rng(2).standard_normal(d.shape) + 0j
    g = prob.Jtvec(v=resid)
    assert g.shape == (prob.nrow,)
    assert rel(g, host_gradient(prob, sv, resid)) <= 1e-10


def test_split_sources_over_two_workers(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    prob, sv, sc = pair(freqs=[3.])
    probh, svh, _ = pair(freqs=[3.], hostGradient=True)
    assert len(prob.system.devices) == 2
    d = sv.dpred()
    assert rel(d, svh.dpred()) <= 1e-12
    resid = np.random.default_rng(3).standard_normal(d.shape) + 0j
    assert rel(prob.Jtvec(v=resid), host_gradient(prob, sv, resid)) <= 1e-10
