"""GPU: HelmBaseProblem.illumination with the wavefields in HBM -- the two energy kernels through the C ABI against an extended-precision evaluation
under the bound derived in tests/illumination_cases.py, then the g6 survey (fixed and moving array, both kinds, store and no store, host path), the
complex64 store against the complex128 one, source batches on two workers, the 2.5-D composite, the receiver side, transfers and solves counted, and
stale fields."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import test_gpu_moving as tm
from tests.illumination_cases import NPATTERN, U_RND, LD, energy_columns, energy_exact, energy_check, energy_entry

pytestmark = pytest.mark.gpu

GOLD = tm.GOLD
rel = tm.rel
P = ctypes.c_void_p
UNROLL, MAX_BLOCKS = 8, 2048            # HELM_ENERGY_UNROLL, HELM_ENERGY_MAX_BLOCKS of csrc/helm_internal.hpp
# N = helm_num_points(op) = nz * nx with nz, nx >= 3, so an operator has neither 1 nor 257 (a prime) cells: the smallest grid stands for the single
# partial wave, and 258 and 259 for "one cell (or a few) into the second workgroup"
GRIDS = [(3, 3), (3, 85), (4, 64), (3, 86), (7, 37)]
BIG = (600, 1000)                       # 600 000 cells > 2048 * 256: the grid-stride loop runs twice
GUARD = 517


@pytest.fixture(scope='module')
def handles(helm_lib):
    'bare operators (no model, nothing assembled) whose only use is their N, their device and their stream'
    made = {}

    def get(grid):
        if grid not in made:
            h = helm_lib.helm_create(0, 0, grid[0], grid[1], 10., 10., 1, None)
            assert h and helm_lib.helm_num_points(h) == grid[0] * grid[1]
            made[grid] = h
        return made[grid]
    yield get
    for h in made.values():
        helm_lib.helm_destroy(h)


def launch(lib, h, fmt, dU, dX, nsrc, ld, alpha, dW, dE):
    if fmt == 'c64':
        return lib.helm_energy_accumulate_c64_device(h, P(dU), P(dX), nsrc, ld, alpha, P(dW) if dW else None, P(dE))
    return lib.helm_energy_accumulate_device(h, P(dU), nsrc, ld, alpha, P(dW) if dW else None, P(dE))


def kernel_case(lib, h, fmt, N, nsrc, cols, seed, pad):
    """One set of columns through one kernel, columns ld = N + pad apart with values between them that would wreck any sum that read them: first with no
    weight onto a zero E, then with a weight, alpha = 0.37 and a non-zero E.  Returns the worst error ratio."""
    import torch
    from zephyr_amd import _lib
    from zephyr_amd.fieldstore import unpack_reference
    dev = torch.device('cuda', 0)
    ld = N + pad
    U = energy_columns(N, cols, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    dUc = torch.from_numpy(np.ascontiguousarray(U.T)).to(dev)
    if fmt == 'c64':
        dPk, dX = torch.empty((nsrc, N), dtype=torch.complex64, device=dev), torch.empty(nsrc, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _lib.check(lib.helm_pack_c64_device(h, P(dUc.data_ptr()), nsrc, N, P(dPk.data_ptr()), P(dX.data_ptr())), h)
        U = unpack_reference(dPk.cpu().numpy().T, dX.cpu().numpy())                 # what the kernel reads, exactly
        dU = torch.full((nsrc, ld), complex(3e18, -3e18), dtype=torch.complex64, device=dev)
        dU[:, :N] = dPk
        xptr = dX.data_ptr()
    else:
        dU = torch.full((nsrc, ld), complex(1e150, -1e150), dtype=torch.complex128, device=dev)
        dU[:, :N] = dUc
        xptr = 0
    worst = 0.0
    for alpha, W in ((1.0, None), (0.37, 10.0 ** rng.uniform(-3, 3, N))):
        E0 = np.zeros(N) if W is None else energy_entry(rng, energy_exact(U, alpha, W))
        exact = energy_exact(U, alpha, W, E0)
        dW = None if W is None else torch.from_numpy(W).to(dev)
        runs = []
        for _ in range(2):
            dE = torch.full((N + 2 * GUARD,), -7.0, dtype=torch.float64, device=dev)
            dE[GUARD:GUARD + N] = torch.from_numpy(E0).to(dev)
            torch.cuda.synchronize(dev)
            _lib.check(launch(lib, h, fmt, dU.data_ptr(), xptr, nsrc, ld, alpha, 0 if dW is None else dW.data_ptr(), dE.data_ptr() + 8 * GUARD), h)
            e = dE.cpu().numpy()
            assert np.all(e[:GUARD] == -7.0) and np.all(e[GUARD + N:] == -7.0)        # the words around E are untouched
            runs.append(e[GUARD:GUARD + N].copy())
        assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))         # the same bits on every run
        bad, ratio = energy_check(runs[0], exact, nsrc)
        assert bad == 0, (fmt, N, nsrc, list(cols), alpha, ratio)
        worst = max(worst, ratio)
    return worst


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['c128', 'c64'])
@pytest.mark.parametrize('nsrc', [1, 5, UNROLL, 13, 67])
@pytest.mark.parametrize('grid', GRIDS)
def test_energy_kernels_against_extended_precision(helm_lib, handles, grid, nsrc, fmt):
    """helm_energy_accumulate_device / _c64_device per cell within (nsrc + 7) 2^-53 of the longdouble value of E + alpha W sum_s |u_s|^2 (the complex64
    form: of the UNPACKED values) -- one column, below, at and above the unroll and no multiple of it; one partial wave, one cell short of a workgroup, a
    full one, a few cells into the second; every kind of column of illumination_cases at every place in the sum."""
    N = grid[0] * grid[1]
    starts = range(NPATTERN) if nsrc == 1 else (0, 3, 5)
    worst = max(kernel_case(helm_lib, handles(grid), fmt, N, nsrc, range(s, s + nsrc), seed=17 * nsrc + s, pad=3) for s in starts)
    print('energy %s N=%d nsrc=%d: worst err / bound = %.3f' % (fmt, N, nsrc, worst))


@pytest.mark.parametrize('fmt', ['c128', 'c64'])
def test_energy_kernels_where_the_grid_stride_loop_runs_twice(helm_lib, handles, fmt):
    N = BIG[0] * BIG[1]
    assert MAX_BLOCKS * 256 < N < 2 * MAX_BLOCKS * 256
    worst = kernel_case(helm_lib, handles(BIG), fmt, N, 3, [0, 5, 8], seed=3, pad=5)
    print('energy %s N=%d nsrc=3: worst err / bound = %.3f' % (fmt, N, worst))


def test_energy_kernels_refuse_bad_arguments(helm_lib, handles):
    import torch
    dev = torch.device('cuda', 0)
    h, N, nsrc = handles((4, 64)), 256, 3
    dU = torch.zeros((nsrc, N + 1), dtype=torch.complex128, device=dev)
    dU32 = torch.zeros((nsrc, N + 1), dtype=torch.complex64, device=dev)
    dX = torch.zeros(nsrc + 1, dtype=torch.int32, device=dev)
    dW, dE = torch.ones(N + 1, dtype=torch.float64, device=dev), torch.zeros(N + 1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    u, u32, x, w, e = dU.data_ptr(), dU32.data_ptr(), dX.data_ptr(), dW.data_ptr(), dE.data_ptr()
    ARG = -1
    f128, f64 = helm_lib.helm_energy_accumulate_device, helm_lib.helm_energy_accumulate_c64_device
    assert f128(h, P(u), nsrc, N, 1.0, P(w), P(e)) == 0 and f64(h, P(u32), P(x), nsrc, N, 1.0, P(w), P(e)) == 0
    assert f128(h, P(u), nsrc, N, 0.0, None, P(e)) == 0                                # (alpha = 0 and no weight are fine)
    for bad in ((None, P(u), nsrc, N, 1.0, P(w), P(e)), (h, None, nsrc, N, 1.0, P(w), P(e)), (h, P(u), nsrc, N, 1.0, P(w), None),
                (h, P(u), 0, N, 1.0, P(w), P(e)), (h, P(u), nsrc, N - 1, 1.0, P(w), P(e)), (h, P(u + 8), nsrc, N, 1.0, P(w), P(e)),
                (h, P(u), nsrc, N, 1.0, P(w + 4), P(e)), (h, P(u), nsrc, N, 1.0, P(w), P(e + 4)), (h, P(u), nsrc, N, -1.0, P(w), P(e)),
                (h, P(u), nsrc, N, -0.5, None, P(e)), (h, P(u), nsrc, N, math.nan, P(w), P(e))):
        assert f128(*bad) == ARG, bad
    for bad in ((None, P(u32), P(x), nsrc, N, 1.0, P(w), P(e)), (h, None, P(x), nsrc, N, 1.0, P(w), P(e)), (h, P(u32), None, nsrc, N, 1.0, P(w), P(e)),
                (h, P(u32), P(x), nsrc, N, 1.0, P(w), None), (h, P(u32), P(x), 0, N, 1.0, P(w), P(e)), (h, P(u32), P(x), nsrc, N - 1, 1.0, P(w), P(e)),
                (h, P(u32 + 4), P(x), nsrc, N, 1.0, P(w), P(e)), (h, P(u32), P(x), nsrc, N, 1.0, P(w + 4), P(e)), (h, P(u32), P(x), nsrc, N, 1.0, P(w), P(e + 4)),
                (h, P(u32), P(x), nsrc, N, -1.0, P(w), P(e)), (h, P(u32), P(x), nsrc, N, math.nan, None, P(e))):
        assert f64(*bad) == ARG, bad
    assert np.all(dE.cpu().numpy() == 0.0)                                              # nothing was launched by a refused call (and the fields were zero)


# ---- the g6 survey -------------------------------------------------------------------------------------------------------------------------
WEIGHT_SLACK = 32


def g6_pair(mode, **kw):
    if mode == 'relative':
        return tm.g6_pair(**kw)
    g, _ = tm.g6_config()
    return tm.g6_pair(geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), **kw)


def exact_rows(prob, fields, kind):
    """(nfreq, N) longdouble: w_f sum_s |fields[f][:, s]|^2 from the fp64 fields given, w_f = omega^4 / |c|^6 for kind pseudoHessian.  The weight is
    evaluated here in extended precision from c and the frequency; the one the code under test uses is made in fp64 -- 1 / (c c c) (two complex products,
    one complex division), its squared modulus, omega = 2 pi f to the fourth power, the product with |scaleTerm|^2 -- which WEIGHT_SLACK = 32 roundings
    cover with room (sqrt(5) u per complex product and 5 u for the division in modulus, doubled by the square: 19 u; 2 u for the sum of squares, 5 u for
    omega^4, 2 u for the products)."""
    rows = []
    for ifreq, uf in enumerate(fields):
        E = energy_exact(uf)
        if kind == 'pseudoHessian':
            c = np.ravel(prob.system.subProblems[ifreq].c).astype(np.complex128)
            omega = 2 * LD(np.pi) * LD(prob.survey.freqs[ifreq])
            E = E * omega ** 4 / (c.real.astype(LD) ** 2 + c.imag.astype(LD) ** 2) ** 3
        rows.append(E)
    return np.stack(rows)


@pytest.mark.parametrize('kind', ['energy', 'pseudoHessian'])
@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_g6_from_the_store_without_a_store_and_on_the_host(helm_lib, monkeypatch, mode, kind):
    """illumination(u=F) within the summed bound of the longdouble evaluation of the downloaded fields (one launch of nsrc columns per frequency onto the same
    partial; the weight of the pseudo-Hessian as exact_rows says), illumination() within twice that of it, the per-frequency rows, the host path to 1e-12"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    _, prob, sv = g6_pair(mode)
    _, probh, _ = g6_pair(mode, hostGradient=True)
    assert prob._deviceGradientAvailable() and not probh._deviceGradientAvailable()
    nf, ns = sv.nfreq, sv.nsrc
    extra = WEIGHT_SLACK if kind == 'pseudoHessian' else 0
    F = prob.fieldsDevice()
    assert F.scale == 1.0                                      # (what F[f] downloads is what the store holds)
    rows = exact_rows(prob, [F[f] for f in range(nf)], kind)
    exact = rows.sum(axis=0)
    HF = prob.illumination(u=F, kind=kind)
    assert HF.shape == (prob.nrow,) and HF.dtype == np.float64 and np.all(HF >= 0) and HF.max() > 0
    bad, worst = energy_check(HF, exact, [ns] * nf, extra=extra)
    print('g6 %s %s: illumination(u=F) worst err / summed bound = %.3f' % (mode, kind, worst))
    assert bad == 0, worst
    RF = prob.illumination(u=F, kind=kind, perFreq=True)
    assert RF.shape == (nf, prob.nrow)
    for f in range(nf):
        assert energy_check(RF[f], rows[f], ns, extra=extra)[0] == 0, f
    H0 = prob.illumination(kind=kind)
    print('g6 %s %s: illumination() bit-identical to illumination(u=F): %s' % (mode, kind, np.array_equal(H0, HF)))
    bound2 = 2 * (nf * (ns + 7) + extra) * U_RND * HF
    assert np.all(np.abs(H0 - HF) <= bound2)
    assert np.array_equal(prob.illumination(u=F, kind=kind), HF)                       # the same bits on every run
    Hh = probh.illumination(kind=kind)
    print('g6 %s %s: host path against device path, rel = %.2e' % (mode, kind, rel(Hh, HF)))
    assert rel(Hh, HF) <= 1e-12
    assert rel(prob.illumination(u=list(F), kind=kind), HF) <= 1e-12                   # host arrays given: the numpy branch on the device problem
    F.release()
    del prob.factors, probh.factors


def test_complex64_store_against_the_complex128_store_within_the_format_bound(helm_lib, monkeypatch):
    """fieldstore_cases.pack_bound_violations states the format: per component |x^ - x| <= 2^-24 |x| where |x| >= thr_s = 2^(e_s - 126), <= thr_s below.
    Where the first holds, x^2 (1 + d)^2 is within (2^-23 + 2^-48) x^2 of x^2; where the second does, |x^| < 2 thr_s and |x^2 - x^2^| = |x^ - x||x^ + x|
    < 3 thr_s^2, twice per value.  So per cell |H64 - H128| <= 2^-22 H128 + sum_f w_f sum_s 3 * 2^(2 (e_s - 126) + 1), the 2^-22 (twice 2^-23) also
    covering the roundings of both sums, (nsrc + 7) 2^-53 per launch."""
    monkeypatch.setenv('HELM_DEVICES', '0')
    _, prob, sv = g6_pair('fixed')
    _, prob64, _ = g6_pair('fixed', fieldsDtype='complex64')
    F, F64 = prob.fieldsDevice(), prob64.fieldsDevice()
    assert F64.dtype == 'complex64'
    for kind in ('energy', 'pseudoHessian'):
        H128, H64 = prob.illumination(u=F, kind=kind), prob64.illumination(u=F64, kind=kind)
        floor = np.zeros(prob.nrow, dtype=LD)
        for _, _, ifreq, c0, _ in F64.items:
            e = F64.slice(ifreq, c0)[1].cpu().numpy().astype(np.int64)
            w = LD(1)
            if kind == 'pseudoHessian':
                w = (np.abs(prob.gradientScaler(ifreq)) ** 2).astype(LD)
            floor = floor + w * (3 * np.ldexp(LD(1), 2 * (e - 126) + 1)).sum()
        err = np.abs(H64.astype(LD) - H128.astype(LD))
        bound = LD(2.0) ** -22 * H128.astype(LD) + floor
        print('complex64 store %s: worst |H64 - H128| / bound = %.3f; rel = %.2e' % (kind, float((err / bound).max()), rel(H64, H128)))
        assert np.all(err <= bound)
        assert rel(H64, H128) > 0                              # (the packed store was read, not a complex128 copy)
        assert np.array_equal(prob64.illumination(u=F64, kind=kind), H64)
    F.release(), F64.release()
    del prob.factors, prob64.factors


def test_two_workers_split_the_sources_and_agree_with_one(helm_lib, monkeypatch):
    'one frequency, two workers on GPU 0 (0:6 / 6:13): two partials summed on the host instead of one sum in order -- within the bound, not the same bits'
    g, _ = tm.g6_config()
    one = dict(freqs=[float(g['freqs'][1])], sterms=g['sterms'][1:2])
    monkeypatch.setenv('HELM_DEVICES', '0')
    _, prob1, sv1 = g6_pair('fixed', **one)
    F1 = prob1.fieldsDevice()
    res1 = {kind: (prob1.illumination(u=F1, kind=kind), prob1.illumination(kind=kind)) for kind in ('energy', 'pseudoHessian')}
    exact = {kind: exact_rows(prob1, [F1[0]], kind)[0] for kind in res1}
    F1.release()
    del prob1.factors
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    _, prob2, sv2 = g6_pair('fixed', **one)
    assert len(prob2.system.devices) == 2
    F2 = prob2.fieldsDevice()
    assert [(w, c0, c1) for w, _, _, c0, c1 in F2.items] == [(0, 0, 6), (1, 6, 13)]
    for kind, (HF1, H01) in res1.items():
        extra = WEIGHT_SLACK if kind == 'pseudoHessian' else 0
        # each partial within (k + 7) u of its part, one host addition more: (7 + 7) + 1 roundings on the larger batch
        for H in (prob2.illumination(u=F2, kind=kind), prob2.illumination(kind=kind)):
            assert energy_check(H, exact[kind], 7 + 1, extra=extra)[0] == 0
            assert np.all(np.abs(H - HF1) <= ((7 + 8) + (13 + 7) + 2 * extra) * U_RND * HF1)
    F2.release()
    del prob2.factors


def test_25d_store_and_solve_agree_with_the_downloaded_ky_sum(helm_lib, monkeypatch):
    'g11, the ky sum formed in HBM by the composite: the energy is that of the ky-summed field, from the store and from a fresh solve'
    import zephyr_amd as za
    from zephyr_amd.problem import Helm25DProblem
    from zephyr_amd.survey import Helm25DSurvey
    monkeypatch.setenv('HELM_DEVICES', '0')
    g = np.load(os.path.join(GOLD, 'g11_25d_survey.npz'))
    nz, nx = g['c'].shape
    sc = dict(nx=nx, nz=nz, dx=10., dz=10., c=g['c'], rho=g['rho'], nPML=6, freqs=list(g['freqs']), Disc=za.MiniZephyr25D, nky=int(g['nky']), parallel=False,
              sterms=g['sterms'], geom=dict(src=g['src'], rec=g['rec'], mode='fixed'), rtol=1e-11)
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    assert prob._deviceGradientAvailable()
    F = prob.fieldsDevice()
    assert F.scale == 1.0                                      # (the composite applies its own scaleTerm inside the ky sum)
    nf, ns = sv.nfreq, sv.nsrc
    fields = [F[f] for f in range(nf)]
    for kind in ('energy', 'pseudoHessian'):
        extra = WEIGHT_SLACK if kind == 'pseudoHessian' else 0
        exact = exact_rows(prob, fields, kind).sum(axis=0)
        HF = prob.illumination(u=F, kind=kind)
        bad, worst = energy_check(HF, exact, [ns] * nf, extra=extra)
        print('2.5-D %s: illumination(u=F) worst err / summed bound = %.3f' % (kind, worst))
        assert bad == 0 and HF.max() > 0
        H0 = prob.illumination(kind=kind)
        print('2.5-D %s: illumination() against illumination(u=F), rel = %.2e' % (kind, rel(H0, HF)))
        assert rel(H0, HF) <= 1e-9                            # (two ky sums of iterative solves at rtol 1e-11: what dpred(u=F) is held to against dpred())
    F.release()
    del prob.factors


@pytest.mark.parametrize('kind', ['energy', 'pseudoHessian'])
def test_receiver_side_matches_the_host_path(helm_lib, monkeypatch, kind):
    monkeypatch.setenv('HELM_DEVICES', '0')
    _, prob, sv = g6_pair('fixed')
    _, probh, _ = g6_pair('fixed', hostGradient=True)
    HR = prob.illumination(kind=kind, side='receiver', perFreq=True)
    Hh = probh.illumination(kind=kind, side='receiver', perFreq=True)
    assert HR.shape == (sv.nfreq, prob.nrow) and np.all(HR >= 0) and HR.max() > 0
    print('receiver side %s: device against host, rel = %.2e' % (kind, rel(HR, Hh)))
    assert rel(HR, Hh) <= 1e-12
    assert rel(HR.sum(axis=0), prob.illumination(kind=kind)) > 1e-3                     # (not the source side)
    _, probr, _ = g6_pair('relative')
    with pytest.raises(ValueError):
        probr.illumination(side='receiver')
    with pytest.raises(ValueError):
        prob.illumination(side='receiver', u=[])
    del prob.factors, probh.factors


def test_counts_no_solve_from_the_store_no_wavefield_comes_down(helm_lib, monkeypatch):
    """Patched as test_counts_fields_solved_once... does: with u=F no solve is issued and 8 N bytes per worker come down; with u=None nsrc columns per
    frequency are solved (nrec for the receiver side) and again only 8 N bytes come down; no host-array solve anywhere."""
    from zephyr_amd import _lib
    from zephyr_amd.discretization import BaseDiscretization
    monkeypatch.setenv('HELM_DEVICES', '0')
    counts = dict(solve=0, cols=[], down=[])
    real_solve, real_sd, real_fd, real_fdp = BaseDiscretization._solve, BaseDiscretization.solveDevice, _lib.from_device, _lib.from_device_pinned

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
    monkeypatch.setattr(BaseDiscretization, '_solve', solve)
    monkeypatch.setattr(BaseDiscretization, 'solveDevice', solve_device)
    monkeypatch.setattr(_lib, 'from_device', counting(real_fd))
    monkeypatch.setattr(_lib, 'from_device_pinned', counting(real_fdp))
    for mode in ('fixed', 'relative'):
        _, prob, sv = g6_pair(mode)
        N, nfreq, nsrc, nrec = prob.nrow, sv.nfreq, sv.nsrc, sv.nrec
        F = prob.fieldsDevice()
        for kind in ('energy', 'pseudoHessian'):
            counts.update(solve=0, cols=[], down=[])
            prob.illumination(u=F, kind=kind)
            assert (counts['solve'], counts['cols'], counts['down']) == (0, [], [8 * N])
            counts.update(cols=[], down=[])
            prob.illumination(u=F, kind=kind, perFreq=True)
            assert (counts['solve'], counts['cols'], counts['down']) == (0, [], [8 * N * nfreq])
            counts.update(cols=[], down=[])
            prob.illumination(kind=kind)
            assert (counts['solve'], counts['cols'], counts['down']) == (0, [nsrc] * nfreq, [8 * N])
        if mode == 'fixed':
            counts.update(cols=[], down=[])
            prob.illumination(side='receiver')
            assert (counts['solve'], counts['cols'], counts['down']) == (0, [nrec] * nfreq, [8 * N])
        F.release()
        del prob.factors


def test_stale_fields_are_refused(helm_lib):
    g, prob, sv = g6_pair('fixed')
    F = prob.fieldsDevice()
    H = prob.illumination(u=F)
    prob.updateModel(g['c'])                                   # the same model: the fields stay good
    assert np.array_equal(prob.illumination(u=F), H)
    with pytest.raises(ValueError):
        prob.illumination(g['c'] * 1.01, u=F)                  # a model handed to illumination itself counts
    with pytest.raises(ValueError):
        prob.illumination(u=F)
    F2 = prob.fieldsDevice(g['c'])
    assert np.array_equal(prob.illumination(u=F2), H)
    F2.release()
    with pytest.raises(ValueError):
        prob.illumination(u=F2)
    with pytest.raises(ValueError):
        prob.illumination(u=F2, side='receiver')
    F.release()
    del prob.factors
