"""Shared cases of the exact multiscale tests (tests/test_multiscale_exact_host.py, tests/test_gpu_multiscale_exact.py): the axis pairs and grid
pairs of the transposed grid transfer, dense restatements of the windows, and the error bound of a transposed application."""
import numpy as np

from zephyr_amd.interpolation import SplineGridInterpolator, regrid_axis, regrid_axis_t

U = 2. ** -53

# (n_in, n_out, h_out) with h_in = 1: the pairs of test_regrid_host.py::test_axis_matches_not_a_knot_spline and two more (W = 64 with WT = 63; an
# integer scale whose transpose has all-zero rows)
AXIS_PAIRS = [
    (4, 9, 0.4), (5, 3, 2.), (57, 20, 2.9), (57, 57, 1.), (1024, 468, 1024 / 468.), (468, 1024, 468 / 1024.), (1024, 102, 1024 / 102.),
    (100, 10, 10.), (10, 100, 0.1), (101, 34, 3.), (34, 101, 1 / 3.), (57, 21, 2.9), (57, 19, 2.9), (1024, 747, 1.37),
    (150, 147, 1.02), (30, 8, 4.),
]

# (name, (nz, nx), scale, (snz, snx) or None for what the interpolator rounds to): the shapes at which the transposed plan can go wrong
GRID_PAIRS = [
    ('noninteger', (40, 57), 2.47, (17, 23)),       # non-integer scale
    ('integer', (30, 36), 4., (8, 9)),              # integer scale: all-zero transposed rows
    ('wide', (150, 130), 1.02, None),               # W = 64, WT = 63: the <64> instantiation
    ('tiles', (24, 600), 2.9, None),                # more than one column tile on the native side
    ('clamped', (57, 57), 2.9, (21, 21)),           # coarse points clamped beyond the fine extent
    ('identity', (33, 41), 1., None),
]


def dense_axis(n_in, h_in, n_out, h_out):
    'the forward axis as a dense (n_out, n_in) matrix and its window width'
    start, taps = regrid_axis(n_in, h_in, n_out, h_out)
    W = taps.shape[1]
    M = np.zeros((n_out, n_in))
    for j in range(n_out):
        M[j, start[j]:start[j] + W] = taps[j]
    return M, W


def dense_axis_t(n_in, h_in, n_out, h_out):
    'the transposed axis as a dense (n_in, n_out) matrix, its windows and their width; asserts the windows are in bounds'
    start, taps = regrid_axis_t(n_in, h_in, n_out, h_out)
    WT = taps.shape[1]
    assert 1 <= WT <= 64
    assert (start >= 0).all() and (start + WT <= n_out).all()
    M = np.zeros((n_in, n_out))
    for j in range(n_in):
        M[j, start[j]:start[j] + WT] = taps[j]
    return M, start, WT


def touched_width(M):
    'widest range of rows of the dense forward axis M that touch one column (1 when nothing does)'
    wt = 1
    for j in range(M.shape[1]):
        i = np.nonzero(M[:, j])[0]
        if i.size:
            wt = max(wt, int(i.max() - i.min() + 1))
    return wt


def interpolator(shape, scale, target=None, **extra):
    'a SplineGridInterpolator of the (nz, nx) grid at 9 m; target (snz, snx): that coarse grid instead of the rounded one'
    sc = dict(nz=shape[0], nx=shape[1], dz=9., dx=9., scale=scale)
    sc.update(extra)
    ds = SplineGridInterpolator(sc)
    if target is not None and (ds.snz, ds.snx) != tuple(target):
        ds._target = (target[1], target[0], 9. * scale, 9. * scale)
    return ds


def dense_axes(ds):
    'dense forward axes (Az (snz, nz), Ax (snx, nx)) of an interpolator and their transposed widths'
    if ds.identity:
        return np.eye(ds.nz), np.eye(ds.nx), 1, 1
    Az, _ = dense_axis(ds.nz, ds.dz, ds.snz, ds.sdz)
    Ax, _ = dense_axis(ds.nx, ds.dx, ds.snx, ds.sdx)
    return Az, Ax, touched_width(Az), touched_width(Ax)


def transposed_core(Az, Ax, fin):
    """T^T fin in numpy.clongdouble for fin (k, snz, snx) by the dense transposed axes, and S = |Tz|^T |fin| |Tx| (what the bound scales with)"""
    L = np.longdouble
    zt, x = Az.T.astype(L), Ax.astype(L)
    fl = fin.astype(np.clongdouble)
    return np.stack([zt @ f @ x for f in fl]), np.stack([np.abs(zt) @ np.abs(f) @ np.abs(x) for f in fl])


def transposed_reference(ds, core, S, gain, beta, prev, mul):
    'out = beta prev + mul (.) (gain T^T fin) from transposed_core, and |mul gain| S; the interpolator\'s own gain (eCons) is part of T'
    g = np.clongdouble(gain) * np.longdouble(ds.gain)
    m = np.ones(core.shape[1:], dtype=np.clongdouble) if mul is None else mul.astype(np.clongdouble).reshape(core.shape[1:])
    ref = m * (g * core)
    if beta != 0.:
        ref = ref + np.longdouble(beta) * prev.astype(np.clongdouble)
    return ref, S * np.abs(m) * abs(g)


def transposed_bound(WTz, WTx, S, beta, prev):
    """Componentwise bound on |out - ref| in modulus (S: the second return of transposed_reference), u = 2^-53, derived as DESIGN.md 5a / 5b derive theirs.  Each pass is a real-weighted fma dot
    product per component: a chain of n fmas is within gamma_n = n u / (1 - n u) of its sum of moduli, and for real weights the two components'
    errors combine to the same factor on the complex moduli (Minkowski).  Two passes of WTz and WTx terms: (1 + gamma_z)(1 + gamma_x) - 1 on
    S = |Tz|^T |in| |Tx|.  Epilogue: two complex products (gain, mul) of at most 3 u each in modulus (2 sqrt 2 u without fma, less with), one fma
    with beta of u on |beta prev| + |v|: 7 u on |mul gain| S and u on |beta prev|; one more u covers the second-order terms."""
    b = (WTz + WTx + 8) * U * S
    if beta != 0.:
        b = b + U * abs(beta) * np.abs(prev)
    return b


# ---- the multiscale problem ------------------------------------------------------------------------------------------------------------------------
# The 40 x 48 model of tests/test_regrid_host.py::oracle_problem, cMin 1500, targetGPW 12.  'noninteger': freqs [6, 25] -> scales 2.31 and 1;
# 'integer': freqs [6.5, 25] with maxScale 2 -> scales exactly 2 and 1 (coarse nodes coincide with every second native node).
NZ, NX, DX, NPML = 40, 48, 9., 5
PROBLEM_CASES = {'noninteger': dict(freqs=[6., 25.]), 'integer': dict(freqs=[6.5, 25.], maxScale=2.)}
TAYLOR_H = (1., 0.5, 0.25, 0.125, 0.0625, 0.03125)          # five halvings
SECOND = 3.5                                                 # the second-order window of tests/test_full_host.py


def problem_config(case='noninteger', mode='fixed', density=True, **extra):
    from zephyr_amd.distributors import MultiGridMultiFreq
    rng = np.random.default_rng(5)
    c = 2000. + 300. * rng.random((NZ, NX))
    rho = 1000. + 200. * rng.random((NZ, NX))
    src = np.array([[100., 60.], [250., 80.]])
    if mode == 'fixed':
        rec = np.stack([np.linspace(40., 380., 7), np.full(7, 300.)], axis=1)
    else:
        rec = np.stack([np.linspace(-60., 70., 7), np.full(7, 200.)], axis=1)          # a streamer below each source, between the nodes of every grid
    sc = dict(nx=NX, nz=NZ, dx=DX, dz=DX, c=c, rho=rho, nPML=NPML, cMin=1500., targetGPW=12., parallel=False, SystemWrapper=MultiGridMultiFreq,
              geom=dict(src=src, rec=rec, mode=mode), multiscaleDerivatives=True)
    sc.update(PROBLEM_CASES[case])
    sc.update(extra)
    if not density:
        del sc['rho']
    return sc


def host_pair(case='noninteger', mode='fixed', hd=False, density=True, **extra):
    'the pairing on the oracle doubles that honour `transposed`, numpy routes and the host matrix of the transfer'
    from tests import adjoint_cases as ac
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    kw = dict(Disc=ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT, hostGradient=True, hostTransfer=True)
    kw.update(extra)
    sc = problem_config(case, mode, density, **kw)
    prob, sv = Helm2DProblem(sc), Helm2DMultiGridSurvey(sc)
    prob.pair(sv)
    return prob, sv, sc


def case_scales():
    from zephyr_amd.distributors import MultiGridHelper
    return {case: MultiGridHelper(problem_config(case)).scales for case in PROBLEM_CASES}


_SCALES = [s for v in case_scales().values() for s in v]
assert any(s != round(s) for s in _SCALES) and any(s == round(s) and s > 1. for s in _SCALES) and any(s == 1. for s in _SCALES)


def everywhere(seed=21, n=NZ * NX):
    'uniform in +-50, non-zero in every native cell (the perturbation of tests/full_cases.py at this size)'
    v = 50. * np.random.default_rng(seed).uniform(-1., 1., n)
    v[np.abs(v) < 1.] = 1.
    return v


def layer_mask(nz, nx, npml=NPML):
    'True in the absorbing layers and on the boundary of an (nz, nx) grid (what tests/frechet_cases.perturbation zeroes)'
    m = np.ones((nz, nx), dtype=bool)
    m[npml:nz - npml, npml:nx - npml] = False
    return m.ravel()


def layer_free(sv, seed=12):
    """a native perturbation of amplitude about 50 whose image on EVERY grid of the survey vanishes in that grid's absorbing layers: a random vector projected
    onto the null space of the layer rows of every down-scaler (a spline samples, so zeros on the native layers alone ring into the coarse ones)"""
    rows, seen = [], set()
    for ds in sv.preProcessors:
        if id(ds) in seen:
            continue
        seen.add(id(ds))
        rows.append(ds.matrix.toarray()[layer_mask(ds.snz, ds.snx)])
    C = np.concatenate(rows)
    w = 50. * np.random.default_rng(seed).uniform(-1., 1., C.shape[1])
    v = w - np.linalg.lstsq(C, C @ w, rcond=None)[0]          # (the minimum-norm solution of C x = C w is the part of w outside the null space)
    for ds in sv.preProcessors:
        assert np.abs((ds.matrix @ v)[layer_mask(ds.snz, ds.snx)]).max() <= 1e-9
    assert np.abs(v).max() > 10.
    return v


def per_frequency_factors(dpred, Jv, x0, v, shape, hs=TAYLOR_H):
    """ratios of successive Taylor remainders ||d(x0 + h v) - d(x0) - h Jv|| per FREQUENCY, (len(hs) - 1, nfreq): a norm over all the data would let the
    frequency with the largest data hide the others, and each frequency lives on a grid of its own"""
    d0 = dpred(x0).reshape(shape)
    J = np.asarray(Jv).reshape(shape)
    rem = []
    for h in hs:
        d = dpred(tuple(a + h * b for a, b in zip(x0, v)) if isinstance(x0, tuple) else x0 + h * v.reshape(x0.shape)).reshape(shape)
        rem.append([np.linalg.norm(d[:, :, i] - d0[:, :, i] - h * J[:, :, i]) for i in range(shape[2])])
    rem = np.array(rem)
    return rem[:-1] / rem[1:]
