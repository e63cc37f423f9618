"""GPU: the exact pseudo-Hessian of a 3-D problem on the device -- the two kernels of csrc/survey3d_hessian.hip against 80-bit evaluations with bounds counted from
their rounded operations (tests/hessian3d_cases.py), and the routes hessian3D=True opens on Helm3DProblem against the host maps of frechet3d.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import survey3d_cases as s3
from tests import survey3d_density_cases as d3c
from tests import hessian3d_cases as hc
from tests.test_gpu_survey3d import ROUTE_DIMS, bits, route_config

pytestmark = pytest.mark.gpu

GRIDS = [(3, 3, 3), (5, 6, 7), (4, 9, 66), (7, 4, 64), (6, 5, 130)]          # a single interior cell; x below, at and past the 64-wide tile; y not a multiple of 4; two x-tiles
MODES = ('buoyancy', 'gardner', 'blocks')
PAD, GUARD = 37, 5
X = dict(kind='pseudoHessian', linearisation='full')


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


# ---- 1. the kernels against 80-bit evaluations ------------------------------------------------------------------------------------------------------------
def coefficient_planes(op, mode):
    'the planes of k_ph3_coefficients on the device over a sentinel, and their host copies'
    import torch
    from zephyr_amd import device_survey3d as d3
    N = op.nrow
    cpl = lambda: torch.full((N,), complex(7.0, -7.0), dtype=torch.complex128, device='cuda:0')
    rea = lambda: torch.full((N,), 7.0, dtype=torch.float64, device='cuda:0')
    planes = [cpl(), rea(), rea()] + ([cpl(), rea()] if mode == 'blocks' else [])
    torch.cuda.synchronize()
    d3.ph3CoefficientsDevice(op, mode, *planes)
    return planes, dict(zip(('A0', 'h', 'S', 'C', 'Smu'), (p.cpu().numpy() for p in planes)))


def check_kernels(op, dims, k, seed, modes=MODES, weights=(True, False), conjs=(True, False)):
    import torch
    from zephyr_amd import device_survey3d as d3
    N = op.nrow
    ld = N + PAD                                              # a leading dimension past N, the padding NaN: nothing of it may enter a sum
    rng = np.random.default_rng(seed)
    U = s3.randc(rng, (k, ld))
    U[:, N:] = np.nan
    Wh = rng.uniform(0.5, 2.0, N)
    dU, dW = _dev(U), _dev(Wh)
    alpha = 0.7
    worst = {}
    for mode in modes:
        planes, got = coefficient_planes(op, mode)
        _, again = coefficient_planes(op, mode)
        for n, (want, bound) in hc.coefficient_reference(op, mode).items():
            assert np.array_equal(bits(got[n]), bits(again[n]))                                   # two launches: the same bits
            worst['%s plane %s' % (mode, n)] = hc.worst(np.abs(got[n].astype(np.clongdouble) - want), bound)
        blocks = mode == 'blocks'
        rows, ldh = (3, N + PAD) if blocks else (1, N)
        for conj in conjs:
            terms = hc.moments_terms(op, np.conj(U[:, :N]) if conj else U[:, :N], mode)
            for weighted in weights:
                H0 = np.full(2 * GUARD + rows * ldh, 3.25)                                        # guard values before, between and after the rows
                for r in range(rows):
                    H0[GUARD + r * ldh:GUARD + r * ldh + N] = rng.standard_normal(N)
                outs = []
                for _ in range(2):
                    H = _dev(H0)
                    torch.cuda.synchronize()
                    d3.ph3MomentsAccumulateDevice(op, dU, k, planes, alpha, dW if weighted else None, H.data_ptr() + 8 * GUARD, blocks=blocks, conj=conj, ldu=ld, ldh=ldh)
                    outs.append(H.cpu().numpy())
                assert np.array_equal(bits(outs[0]), bits(outs[1]))                               # two runs: the same bits
                body = np.zeros(H0.size, dtype=bool)
                for r in range(rows):
                    body[GUARD + r * ldh:GUARD + r * ldh + N] = True
                assert np.array_equal(bits(outs[0][~body]), bits(H0[~body]))                      # nothing written outside the rows
                assert np.all(np.isfinite(outs[0]))                                               # the NaN padding entered nothing
                take = lambda a: np.stack([a[GUARD + r * ldh:GUARD + r * ldh + N] for r in range(rows)]) if blocks else a[GUARD:GUARD + N]
                want, bound = hc.moments_reference(terms, k, alpha, Wh if weighted else None, take(H0))
                worst['%s conj=%d W=%d' % (mode, conj, weighted)] = hc.worst(np.abs(take(outs[0]).astype(np.longdouble) - want), bound)
    print('%s k=%d: worst error / bound %s' % (dims, k, {n: '%.3f' % v for n, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('dims', GRIDS, ids=lambda d: 'x'.join(map(str, d)))
def test_kernels_against_extended_precision(helm_lib, dims, k):
    import zephyr_amd as za
    op = za.Helm3D(d3c.small_config(dims, seed=k))
    check_kernels(op, dims, k, 100 * k + sum(dims))
    del op.factors


def test_column_loop_and_double_buffer_turn_over_many_times(helm_lib):
    "173 columns on (6, 5, 130): every workgroup walks all of them (gridDim.y == 1), the two buffers change places 172 times"
    import zephyr_amd as za
    dims = (6, 5, 130)
    op = za.Helm3D(d3c.small_config(dims, seed=5))
    check_kernels(op, dims, 173, 77, modes=('blocks', 'gardner'), weights=(False,), conjs=(True,))
    del op.factors


def test_entry_points_exist_and_refuse_what_the_laplacian_kernels_refuse(helm_lib):
    import torch
    import zephyr_amd as za
    from zephyr_amd import _lib
    assert hasattr(helm_lib, 'helm_ph3_coefficients_device') and hasattr(helm_lib, 'helm_ph3_moments_accumulate_device')
    dims = (6, 5, 70)
    op = za.Helm3D(d3c.small_config(dims, seed=9))
    N = op.nrow
    big = torch.zeros(8 * N, dtype=torch.complex128, device='cuda:0')
    b = big.data_ptr()
    P_ = lambda off: ctypes.c_void_p(b + off)
    co, mo = helm_lib.helm_ph3_coefficients_device, helm_lib.helm_ph3_moments_accumulate_device
    # (U at 0, A0 at 16 N, h at 32 N, S at 40 N, C at 48 N, Smu at 64 N, H at 72 N .. 96 N)
    good = lambda h=op.handle, **kw: mo(h, kw.get('U', P_(0)), kw.get('k', 1), kw.get('ld', N), 1, kw.get('blocks', 0), kw.get('A0', P_(16 * N)), P_(32 * N), P_(40 * N),
                                        kw.get('C', P_(48 * N)), P_(64 * N), 1.0, kw.get('W', None), kw.get('H', P_(72 * N)), kw.get('ldh', N))
    assert co(op.handle, 2, P_(16 * N), P_(32 * N), P_(40 * N), P_(48 * N), P_(64 * N)) == 0 and good() == 0 and good(blocks=1) == 0
    assert good(ld=N - 1) == -1                                                    # ld < N
    assert good(k=0) == -1                                                         # no columns
    assert good(U=P_(8)) == -1                                                     # U misaligned
    assert good(H=P_(72 * N + 4)) == -1                                            # H misaligned
    assert good(H=P_(0)) == -1                                                     # H over U
    assert good(H=P_(16 * N)) == -1                                                # H over a plane
    assert good(blocks=1, ldh=N - 1) == -1                                         # ldh < N
    assert good(blocks=1, C=None) == -1                                            # a plane of the blocks missing
    assert good(A0=None) == -1
    assert co(op.handle, 3, P_(16 * N), P_(32 * N), P_(40 * N), None, None) == -1  # no such mode
    assert co(op.handle, 2, P_(16 * N), P_(32 * N), P_(40 * N), None, None) == -1  # the planes of the blocks missing
    assert co(op.handle, 0, P_(16 * N), P_(16 * N), P_(40 * N), None, None) == -1  # overlapping planes
    # a 2-D handle is refused by both
    mz = za.MiniZephyr(dict(nx=20, nz=24, dx=10., c=2500., freq=10., nPML=5))
    assert co(mz.handle, 0, P_(16 * N), P_(32 * N), P_(40 * N), None, None) == -4
    assert '3-D' in _lib.last_error(mz.handle)
    assert mo(mz.handle, P_(0), 1, 480, 1, 0, P_(16 * N), P_(32 * N), P_(40 * N), None, None, 1.0, None, P_(72 * N), 480) == -4
    # a handle that is not assembled
    raw = helm_lib.helm_create3d(0, 6, 5, 70, 9., 11., 10., 2)
    try:
        assert co(raw, 0, P_(16 * N), P_(32 * N), P_(40 * N), None, None) == -3
        assert 'not assembled' in _lib.last_error(raw)
        assert good(h=raw) == -3
    finally:
        helm_lib.helm_destroy(raw)
    del op.factors, mz.factors


# ---- 2. the routes ----------------------------------------------------------------------------------------------------------------------------------------
_ROUTES = {}


def device_pair(mode, gardner=False, **extra):
    import zephyr_amd as za
    sc = dict(route_config(mode), derivatives3D=True, hessian3D=True)
    sc.update(extra)
    if gardner:
        del sc['rho']
    prob, sv = za.Helm3DProblem(sc), za.Helm3DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def routes(mode, gardner=False):
    'one device pair per receiver mode and density convention for the module, with its stored fields'
    if (mode, gardner) not in _ROUTES:
        prob, sv = device_pair(mode, gardner)
        _ROUTES[(mode, gardner)] = dict(prob=prob, sv=sv, F=prob.fieldsDevice())
    return _ROUTES[(mode, gardner)]


CALLS = [('rho', False, 'illumination', dict(parameter='rho')), ('c', False, 'illumination', dict(parameter='c')), ('blocks', False, 'hessianBlocks', {}),
         ('gardner', True, 'illumination', dict(parameter='c'))]


def host_rows(prob, Fh, label):
    """(rows, majorants), one per frequency: |st|^2 times the host maps of frechet3d.py on the downloaded fields -- what Helm3DProblem forms without a GPU"""
    from zephyr_amd import frechet3d
    st = complex(prob.system.scaleTerm)
    a2 = st.real * st.real + st.imag * st.imag
    rows, majs = [], []
    for i, op in enumerate(prob.system.subProblems):
        uh = np.conj(Fh[i] / st)
        for mag, out in ((False, rows), (True, majs)):
            if label == 'blocks':
                out.append(a2 * frechet3d.pseudoHessianBlocks3(op, uh, magnitude=mag))
            else:
                out.append(a2 * frechet3d.pseudoHessianDiagonal3(op, uh, 'rho' if label == 'rho' else 'c', frechet3d.gardnerChain3(op) if label == 'gardner' else None,
                                                                  magnitude=mag))
    return np.stack(rows), np.stack(majs)


@pytest.mark.parametrize('mode', ['fixed', 'relative'])
def test_device_routes_against_the_host_maps_on_the_same_fields(helm_lib, mode):
    """u=F on the device against the host maps fed the DOWNLOADED fields, per frequency and summed, inside the bound of the kernels (two fp64 evaluations:
    host_bound); perFreq rows sum to the total; repeated calls give the same bits"""
    for label, gardner, name, kw in CALLS:
        R_ = routes(mode, gardner)
        prob, sv, F = R_['prob'], R_['sv'], R_['F']
        assert prob._deviceGradientAvailable()
        call = getattr(prob, name)
        Fh = [F[i] for i in range(sv.nfreq)]
        want, maj = host_rows(prob, Fh, label)
        rows, total = call(None, u=F, perFreq=True, **kw, **X), call(None, u=F, **kw, **X)
        N = prob.nrow
        assert rows.dtype == np.float64 and rows.shape == ((sv.nfreq, 3, N) if label == 'blocks' else (sv.nfreq, N)) and total.shape == rows.shape[1:]
        k = sv.nsrc
        w_rows = hc.worst(np.abs(rows - want), hc.host_bound(k, maj))
        w_tot = hc.worst(np.abs(total - want.sum(axis=0)), hc.host_bound(k, maj.sum(axis=0)) + 2 * s3.U53 * np.abs(want).sum(axis=0))
        print('%s %s: device against the host maps on the same fields, worst error / bound %.3f per frequency, %.3f summed' % (mode, label, w_rows, w_tot))
        assert w_rows <= 1.0 and w_tot <= 1.0
        assert np.all(np.abs(rows.sum(axis=0) - total) <= 4 * s3.U53 * np.abs(rows).sum(axis=0))
        assert np.array_equal(bits(call(None, u=F, **kw, **X)), bits(total))
        if label == 'blocks':
            assert np.all(rows[:, 1] ** 2 <= rows[:, 0] * rows[:, 2] * (1 + 1e-12))


def test_velocity_with_an_explicit_density_launches_neither_kernel(helm_lib, monkeypatch):
    from zephyr_amd import device_survey3d as d3
    R_ = routes('fixed')
    prob, F = R_['prob'], R_['F']

    def refuse(*a, **k_):
        raise AssertionError('the closed form of the velocity diagonal launched a kernel of survey3d_hessian.hip')
    want = prob.illumination(None, u=F, parameter='c', **X)
    monkeypatch.setattr(d3, 'ph3MomentsAccumulateDevice', refuse)
    monkeypatch.setattr(d3, 'ph3CoefficientsDevice', refuse)
    assert np.array_equal(bits(prob.illumination(None, u=F, parameter='c', **X)), bits(want))
    assert np.array_equal(bits(prob.illumination(None, u=F, kind='pseudoHessian', linearisation='operator', parameter='c')), bits(want))
    with pytest.raises(AssertionError, match='launched a kernel'):
        prob.illumination(None, u=F, parameter='rho', **X)


def test_scaler_illumination_gives_the_same_bits_before_and_after_an_exact_call(helm_lib):
    R_ = routes('fixed')
    prob, F = R_['prob'], R_['F']
    before = {kind: prob.illumination(None, u=F, kind=kind) for kind in ('energy', 'pseudoHessian')}
    prob.illumination(None, u=F, parameter='rho', **X)
    prob.hessianBlocks(None, u=F, **X)
    for kind, H in before.items():
        assert np.array_equal(bits(prob.illumination(None, u=F, kind=kind)), bits(H))


# Two solves of one system at rtol = 1e-9 give fields that agree to 4e-9 (solver repeatability); H is quadratic in the fields, so two evaluations
# on fields of two solves agree to 8e-9 of the majorant's size -- taken normwise as 1e-7.  Fresh pairs have the same history and usually agree far better.
REPEAT = 1e-7


def test_u_none_against_stored_fields_on_fresh_pairs(helm_lib):
    out = []
    for stored in (True, False):
        prob, sv = device_pair('relative')
        F = prob.fieldsDevice() if stored else None
        out.append((prob.illumination(None, u=F, parameter='rho', **X), prob.hessianBlocks(None, u=F, **X)))
        del prob.factors
    e = [s3.rel(out[1][j], out[0][j]) for j in range(2)]
    print('u=None against u=F on fresh pairs: rho diagonal %.2e, blocks %.2e' % tuple(e))
    assert max(e) <= REPEAT


def test_two_workers_split_the_sources_of_one_frequency(helm_lib, monkeypatch):
    'one frequency, two workers on GPU 0 (columns 0:1 / 1:3): two partials over fewer columns summed on the host instead of one sum in order, on fields of its own solves'
    R_ = routes('fixed')
    want = (R_['prob'].illumination(None, u=R_['F'], parameter='rho', perFreq=True, **X)[0], R_['prob'].hessianBlocks(None, u=R_['F'], perFreq=True, **X)[0])
    sc = route_config('fixed')
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    prob, sv = device_pair('fixed', parallel=True, freqs=sc['freqs'][:1], sterms=sc['sterms'][:1])
    assert len(prob.system.devices) == 2
    F = prob.fieldsDevice()
    assert [(w, c0, c1) for w, _, _, c0, c1 in F.items] == [(0, 0, 1), (1, 1, 3)]
    got = (prob.illumination(None, u=F, parameter='rho', **X), prob.hessianBlocks(None, u=F, **X), prob.illumination(None, parameter='rho', **X))
    e = [s3.rel(got[0], want[0]), s3.rel(got[1], want[1]), s3.rel(got[2], want[0])]
    print('two workers against one: rho diagonal %.2e, blocks %.2e, rho diagonal with u=None %.2e' % tuple(e))
    assert max(e) <= REPEAT
    F.release()
    del prob.factors


# ---- 3. ranks -----------------------------------------------------------------------------------------------------------------------------------------------
RANKS = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
os.environ['HELM_DEVICES'] = '0'
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import survey3d_cases as s3
from tests.test_gpu_hessian3d import device_pair, REPEAT
ref, sref = device_pair('relative', shardFreqs=False)
prob, sv = device_pair('relative')
assert prob._deviceGradientAvailable() and prob.ownedFreqs == [dist.get_rank()] and ref.ownedFreqs == [0, 1]
X = dict(kind='pseudoHessian', linearisation='full')
F = prob.fieldsDevice()
e = [s3.rel(prob.illumination(None, u=F, parameter='rho', perFreq=True, **X), ref.illumination(None, parameter='rho', perFreq=True, **X)),
     s3.rel(prob.hessianBlocks(None, u=F, **X), ref.hessianBlocks(None, **X))]
print('RANK', dist.get_rank(), ['%%.2e' %% x for x in e], flush=True)
ok = max(e) <= REPEAT
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result(helm_lib, tmp_path):
    "the two frequencies sharded over two ranks on one GPU: ONE all-reduce gives every rank the single-rank diagonal (per frequency) and blocks"
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'ranks.py'
    script.write_text(RANKS % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29679', WORLD_SIZE='2', PYTHONPATH=root)
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
