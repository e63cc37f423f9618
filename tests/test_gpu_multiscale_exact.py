"""GPU: the transposed grid transfer (helm_regrid_create_t through `ds.adjoint`) against the product by the dense transposed axes in
numpy.longdouble, at the shapes where the plan can go wrong; the pair identity <S x, y> = <x, S^T y>; forward results keep their bits."""
import numpy as np
import pytest

from tests.multiscale_exact_cases import GRID_PAIRS, dense_axes, interpolator, transposed_bound, transposed_core, transposed_reference

pytestmark = pytest.mark.gpu


def cfields(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def to_layout(a, layout):
    'a (k, N) numpy block as the contiguous array of the layout'
    return np.ascontiguousarray(a if layout == 'kN' else a.T)


@pytest.mark.parametrize('name,shape,scale,target', GRID_PAIRS, ids=[g[0] for g in GRID_PAIRS])
def test_transposed_transfer_within_its_bound(helm_lib, name, shape, scale, target):
    import torch
    dev = torch.device('cuda', 0)
    ds = interpolator(shape, scale, target, eCons=True, device=0)
    if target is not None:
        assert (ds.snz, ds.snx) == target
    Az, Ax, WTz, WTx = dense_axes(ds)
    adj = ds.adjoint
    nat, coarse = (ds.nz, ds.nx), (ds.snz, ds.snx)
    N, Nf = adj.shape
    assert (N, Nf) == (nat[0] * nat[1], coarse[0] * coarse[1])
    if name == 'wide':
        assert max(WTz, WTx) > 32                                 # the <64> instantiation of the column pass
    if name == 'tiles':
        assert ds.nx > 512                                        # several column tiles on the native side
    if name == 'integer':
        assert (~Az.any(axis=0)).sum() > 0                        # all-zero transposed rows
    rng = np.random.default_rng(11)
    gain = 0.5 - 0.25j
    worst = 0.
    for k in (1, 2, 5):
        fin = cfields(rng, k, Nf)
        prev = cfields(rng, k, N)
        mulv = cfields(rng, N)
        core, S0 = transposed_core(Az, Ax, fin.reshape((k,) + coarse))
        for layout in ('kN', 'Nk'):
            for beta in (0., 1.):
                for mul in (None, mulv):
                    dIn = torch.from_numpy(to_layout(fin, layout)).to(dev)
                    dOut = torch.from_numpy(to_layout(prev, layout)).to(dev)
                    dMul = None if mul is None else torch.from_numpy(mul).to(dev)
                    adj.apply_device(dIn, dOut, k=k, gain=gain, beta=beta, mul=dMul, layout=layout)
                    got = dOut.cpu().numpy()
                    got = (got if layout == 'kN' else got.T).reshape((k,) + nat)
                    ref, S = transposed_reference(ds, core, S0, gain, beta, prev.reshape((k,) + nat), mul)
                    bound = transposed_bound(WTz, WTx, S, beta, prev.reshape((k,) + nat))
                    err = np.abs(got.astype(np.clongdouble) - ref)
                    assert np.all(err[bound == 0] == 0)
                    ratio = float((err[bound > 0] / bound[bound > 0]).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1., (k, layout, beta, mul is not None, ratio)
    print('%s: WTz = %d, WTx = %d, worst |out - ref| / bound = %.3f' % (name, WTz, WTx, worst))


@pytest.mark.parametrize('name,shape,scale,target', GRID_PAIRS, ids=[g[0] for g in GRID_PAIRS])
def test_pair_identity_and_host_arrays(helm_lib, name, shape, scale, target):
    ds = interpolator(shape, scale, target, device=0)
    Az, Ax, _, _ = dense_axes(ds)
    N, Nf = ds.adjoint.shape
    rng = np.random.default_rng(5)
    x, y = cfields(rng, N), cfields(rng, Nf)
    Sx, STy = ds * x, ds.adjoint * y                               # host arrays through the plans of the device
    lhs, rhs = np.vdot(y, Sx), np.vdot(STy, x)
    terms = float(np.abs(y) @ (np.kron(np.abs(Az), np.abs(Ax)) @ np.abs(x)))
    print('%s: |<Sx, y> - <x, S^T y>| / sum |terms| = %.2e' % (name, abs(lhs - rhs) / terms))
    assert abs(lhs - rhs) <= 1e-13 * terms
    if not ds.identity:
        S = ds.matrix
        assert np.abs(STy - S.T @ y).max() <= 1e-13 * np.abs(S.T @ np.abs(y)).max()
        real = ds.adjoint * y.real                                # real in, real out; (N_f, k) blocks
        assert real.dtype == np.float64 and real.shape == (N,)
        two = ds.adjoint * np.stack([y, 2 * y], axis=1)
        assert two.shape == (N, 2) and np.array_equal(two[:, 0], STy)


def test_forward_keeps_its_bits_beside_a_transposed_plan(helm_lib):
    import torch
    dev = torch.device('cuda', 0)
    ds = interpolator((61, 83), 2.37, device=0)                    # (a grid pair no other test of this module has planned)
    rng = np.random.default_rng(8)
    f = cfields(rng, 3, ds.shape[1])
    dIn = torch.from_numpy(f).to(dev)

    def forward():
        out = torch.empty((3, ds.shape[0]), dtype=torch.complex128, device=dev)
        ds.apply_device(dIn, out, k=3, gain=1.5 + 0.5j)
        return out.cpu().numpy(), ds * np.ascontiguousarray(f.T)

    before = forward()
    g = torch.from_numpy(cfields(rng, 3, ds.shape[0])).to(dev)
    back = torch.zeros((3, ds.shape[1]), dtype=torch.complex128, device=dev)
    ds.adjoint.apply_device(g, back, k=3)
    assert ds.adjoint.plan(0) != ds.plan(0) and ds.adjoint.plan(0) != ds.T.plan(0)
    after = forward()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert float(back.abs().max()) > 0


def test_up_sampling_transfer_has_no_transposed_plan(helm_lib):
    up = interpolator((101, 101), 3., device=0).T                  # 34 -> 101 per axis: an input node is read by 98 outputs
    with pytest.raises(NotImplementedError):
        up.adjoint * np.zeros(up.shape[0])


# ---- the exact derivatives of a multiscale pairing through the device routes ---------------------------------------------------------------------------
from tests import adjoint_cases as ac                     # noqa: E402
from tests import multiscale_exact_cases as mc            # noqa: E402

FULL, OP, T = dict(linearisation='full'), dict(linearisation='operator'), dict(adjoint='transpose')
PARS = [('full', 'c'), ('full', 'rho'), ('full', 'joint'), ('operator', 'c'), ('operator', 'joint')]
CONFIGS = ['moving', 'fixed', 'noninteger']


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def device_config(name, density=True, **extra):
    """the multigrid_config() geometry of tests/test_moving_plan.py (80 x 96, scales 6, 3 and 1, a streamer that moves with the source) with a density and the key;
    'fixed': the same with a fixed receiver line; 'noninteger': frequencies 7 and 30 Hz, scales 2.57 and 1"""
    import zephyr_amd as za
    from tests.test_moving_plan import multigrid_config
    sc = multigrid_config()
    rng = np.random.default_rng(9)
    sc.update(rho=1000. + 500. * rng.random((sc['nz'], sc['nx'])), Disc=za.MiniZephyr, SystemWrapper=za.MultiGridMultiFreq, multiscaleDerivatives=True, rtol=1e-11)
    if name == 'fixed':
        rec = np.stack([np.linspace(100., 850., 6), np.full(6, 650.)], axis=1)
        sc['geom'] = dict(sc['geom'], rec=rec, mode='fixed')
    elif name == 'noninteger':
        sc['freqs'] = [7., 30.]
    sc.update(extra)
    if not density:
        del sc['rho']
    return sc


def device_pair(name, density=True, **extra):
    from zephyr_amd.problem import Helm2DProblem
    from zephyr_amd.survey import Helm2DMultiGridSurvey
    sc = device_config(name, density, **extra)
    prob, sv = Helm2DProblem(sc), Helm2DMultiGridSurvey(sc)
    prob.pair(sv)
    return prob, sv, sc


def inputs(prob, sv, par, seed=31):
    rng = np.random.default_rng(seed)
    n = 2 * prob.nrow if par == 'joint' else prob.nrow
    return rng.standard_normal(n), rng.standard_normal(n), ac.randc(rng, sv.nD)


@pytest.mark.parametrize('name', CONFIGS)
def test_device_routes_against_the_host_route_fed_the_downloaded_fields(helm_lib, monkeypatch, name):
    """complex128 store: the device pipelines against the numpy route of the same pairing (hostGradient) fed the per-grid fields downloaded from the store, 1e-12;
    the adjoint identity on the device at 1e-10; u = None and a second call give the bits of u = F; dpred(u=F) is dpred()"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, _ = device_pair(name)
    probh, svh, _ = device_pair(name, hostGradient=True)
    assert prob._deviceGradientAvailable() and not probh._deviceGradientAvailable()
    scales = sv.mgHelper.scales
    assert scales == [6., 3., 1.] if name != 'noninteger' else (abs(scales[0] - 18. / 7.) < 1e-12 and scales[1] == 1.)
    F = prob.fieldsDevice()
    subs = prob.system.subProblems
    uF = [F[i] for i in range(sv.nfreq)]
    assert [u.shape for u in uF] == [(int(op.nz) * int(op.nx), sv.nsrc) for op in subs]            # every frequency's fields on ITS grid
    assert sum(F.nbytes.values()) == 16 * sv.nsrc * sum(int(op.nrow) for op in subs)
    d = sv.dpred()
    assert ac.rel(sv.dpred(u=F), d) <= 1e-12
    worst = 0.
    for lin, par in PARS:
        v, p, r = inputs(prob, sv, par)
        kw, kh = dict(u=F, linearisation=lin, parameter=par), dict(u=uF, linearisation=lin, parameter=par)
        gT, Jv = prob.Jtvec(None, r, **kw, **T), prob.JvecBorn(None, v, **kw)
        assert gT.shape == v.shape and gT.dtype == np.float64 and Jv.shape == (sv.nD,) and Jv.dtype == np.complex128
        shape = (sv.nrec, sv.nsrc, sv.nfreq)
        Jh = probh.JvecBorn(None, v, **kh)
        eg = ac.rel(gT, probh.Jtvec(None, r, **kh, **T))
        ej = max(ac.rel(Jv.reshape(shape)[:, :, i], Jh.reshape(shape)[:, :, i]) for i in range(sv.nfreq))          # (per frequency: each lives on a grid of its own)
        lhs = ac.inner(Jv, r)
        miss = abs(lhs - ac.inner(v, gT)) / abs(lhs)
        if (lin, par) == ('full', 'joint'):
            # one frequency's residual at a time, so that the frequency with the largest data does not hide the coarse grids
            for i in range(sv.nfreq):
                ri = np.zeros(shape, dtype=np.complex128)
                ri[:, :, i] = r.reshape(shape)[:, :, i]
                gi = prob.Jtvec(None, ri.ravel(), **kw, **T)
                li = ac.inner(Jv, ri)
                eg = max(eg, ac.rel(gi, probh.Jtvec(None, ri.ravel(), **kh, **T)))
                miss = max(miss, abs(li - ac.inner(v, gi)) / abs(li))
        print('%s %s %s: Jtvec against the host route %.2e, JvecBorn %.2e; identity misses by %.2e' % (name, lin, par, eg, ej, miss))
        worst = max(worst, eg, ej)
        assert eg <= 1e-12 and ej <= 1e-12
        assert miss <= 1e-10
        assert np.array_equal(bits(prob.Jtvec(None, r, **kw, **T)), bits(gT))                      # (twice: the same bits)
        if (lin, par) in (('full', 'c'), ('full', 'joint')):
            kn = dict(linearisation=lin, parameter=par)
            assert np.array_equal(bits(prob.Jtvec(None, r, **kn, **T)), bits(gT))                  # (u = None: solved, used, released)
            assert np.array_equal(bits(prob.JvecBorn(None, v, **kn)), bits(Jv))
            Hp = prob.Hvec(None, p, **kw)
            eh = ac.rel(Hp, probh.Hvec(None, p, **kh))
            print('%s %s %s: Hvec against the host route %.2e' % (name, lin, par, eh))
            assert Hp.dtype == np.float64 and eh <= 1e-12 and float(p @ Hp) > 0
    F.release()
    del prob.factors, probh.factors


def test_complex64_store_against_the_host_route_on_the_unpacked_fields(helm_lib, monkeypatch):
    "the tolerance of the sibling tests of that store (tests/test_gpu_full.py): 1e-6 against the host route on the same, unpacked fields, the identity at 1e-7"
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, _ = device_pair('moving', fieldsDtype='complex64')
    probh, svh, _ = device_pair('moving', hostGradient=True)
    F = prob.fieldsDevice()
    assert F.dtype == 'complex64'
    uF = list(F)
    assert ac.rel(sv.dpred(u=F), sv.dpred()) <= 1e-6
    for lin, par in (('full', 'c'), ('full', 'joint')):
        v, _, r = inputs(prob, sv, par)
        kw, kh = dict(u=F, linearisation=lin, parameter=par), dict(u=uF, linearisation=lin, parameter=par)
        gT, Jv = prob.Jtvec(None, r, **kw, **T), prob.JvecBorn(None, v, **kw)
        eg, ej = ac.rel(gT, probh.Jtvec(None, r, **kh, **T)), ac.rel(Jv, probh.JvecBorn(None, v, **kh))
        lhs = ac.inner(Jv, r)
        miss = abs(lhs - ac.inner(v, gT)) / abs(lhs)
        print('complex64 %s %s: Jtvec %.2e, JvecBorn %.2e, identity %.2e' % (lin, par, eg, ej, miss))
        assert eg <= 1e-6 and ej <= 1e-6 and miss <= 1e-7
    F.release()
    del prob.factors, probh.factors


@pytest.mark.parametrize('name,density', [('moving', True), ('noninteger', False)], ids=['moving-rho', 'noninteger-gardner'])
def test_taylor_remainder_of_the_device_dpred_falls_at_second_order_on_every_grid(helm_lib, monkeypatch, name, density):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, sc = device_pair(name, density)
    c0 = np.array(sc['c'], dtype=np.float64)
    v = mc.everywhere(21, prob.nrow)
    Jv = prob.JvecBorn(c0, v, **FULL)
    r = ac.randc(np.random.default_rng(2), sv.nD)
    lhs = ac.inner(Jv, r)
    miss = abs(lhs - ac.inner(v, prob.Jtvec(None, r, **FULL, **T))) / abs(lhs)          # (the Gardner chain at c_f on both sides)
    print('device %s %s: identity misses by %.2e' % (name, 'rho' if density else 'gardner', miss))
    assert miss <= 1e-10
    f = mc.per_frequency_factors(lambda c: sv.dpred(c), Jv, c0, v, (sv.nrec, sv.nsrc, sv.nfreq))
    print('device %s %s: factors per frequency %s' % (name, 'rho' if density else 'gardner', np.round(f.T, 3).tolist()))
    assert np.all(f >= mc.SECOND)
    del prob.factors


def test_two_workers_split_the_sources(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    one, sv1, _ = device_pair('moving', freqs=[6.])
    v, _, r = inputs(one, sv1, 'joint')
    g1, d1 = one.Jtvec(None, r, parameter='joint', **FULL, **T), one.JvecBorn(None, v, parameter='joint', **FULL)
    del one.factors
    monkeypatch.setenv('HELM_DEVICES', '0,0')
    two, sv2, _ = device_pair('moving', freqs=[6.])
    assert len(two.system.devices) == 2
    F = two.fieldsDevice()
    assert len(F.items) == 2
    g2, d2 = two.Jtvec(None, r, u=F, parameter='joint', **FULL, **T), two.JvecBorn(None, v, u=F, parameter='joint', **FULL)
    print('two workers: Jtvec %.2e, JvecBorn %.2e' % (ac.rel(g2, g1), ac.rel(d2, d1)))
    assert ac.rel(g2, g1) <= 1e-12 and ac.rel(d2, d1) <= 1e-12
    F.release()
    del two.factors


def test_the_mux_routes_keep_their_bits_and_the_key_is_an_opt_in(helm_lib, monkeypatch):
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, sc = device_pair('moving')
    _, _, r = inputs(prob, sv, 'c')
    g0, d0 = prob.Jtvec(None, r), sv.dpred()
    prob.Jtvec(None, r, **FULL, **T)
    prob.Hvec(None, np.ones(prob.nrow), **FULL)
    assert np.array_equal(bits(prob.Jtvec(None, r)), bits(g0)) and np.array_equal(bits(sv.dpred()), bits(d0))
    del prob.factors
    off, svo, _ = device_pair('moving', multiscaleDerivatives=False)
    with pytest.raises(NotImplementedError, match='fieldsDevice serves single-grid surveys'):
        off.fieldsDevice()
    with pytest.raises(NotImplementedError, match='serves single-grid surveys'):
        off.Jtvec(None, r, **FULL, **T)
    assert np.array_equal(bits(off.Jtvec(None, r)), bits(g0)) and np.array_equal(bits(svo.dpred()), bits(d0))
    del off.factors


def test_the_per_grid_store_is_refused_where_native_grid_fields_are_read(helm_lib, monkeypatch):
    """the reference's u-given gradient and the 'scaler' illumination kinds multiply native-grid fields: handed the per-grid store they raise, they do not image
    coarse rows into the native partial; with u=None they are what they are without the key, bit for bit"""
    monkeypatch.setenv('HELM_DEVICES', '0')
    prob, sv, _ = device_pair('moving')
    off, svo, _ = device_pair('moving', multiscaleDerivatives=False)
    _, _, r = inputs(prob, sv, 'c')
    F = prob.fieldsDevice()
    for call in (lambda: prob.Jtvec(None, r, u=F), lambda: prob.illumination(u=F, kind='energy'), lambda: prob.illumination(u=F, kind='pseudoHessian'),
                 lambda: prob.illumination(u=F, kind='energy', perFreq=True)):
        with pytest.raises(NotImplementedError, match='per-grid store'):
            call()
    with pytest.raises(NotImplementedError, match="'scaler'"):
        prob.Jtvec(None, r, u=F, **T)
    assert ac.rel(sv.dpred(u=F), sv.dpred()) <= 1e-12                                                    # (the store still serves what reads it per grid)
    F.release()
    for kind in ('energy', 'pseudoHessian'):
        assert np.array_equal(bits(prob.illumination(kind=kind)), bits(off.illumination(kind=kind)))
    assert np.array_equal(bits(prob.Jtvec(None, r)), bits(off.Jtvec(None, r)))
    uN = prob.fields()                                                                                   # (native-grid host fields: the route as it was)
    assert np.array_equal(bits(prob.Jtvec(None, r, u=uN)), bits(off.Jtvec(None, r, u=uN)))
    del prob.factors, off.factors


RANKS = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r)
os.environ['HELM_DEVICES'] = '0'
import torch.distributed as dist
dist.init_process_group('gloo', rank=int(os.environ['RANK']), world_size=int(os.environ['WORLD_SIZE']))
from tests import adjoint_cases as ac
from tests.test_gpu_multiscale_exact import device_pair, inputs
ref, sref, _ = device_pair('moving', shardFreqs=False)
prob, sv, _ = device_pair('moving')
assert prob._deviceGradientAvailable() and prob.ownedFreqs == list(range(dist.get_rank(), 3, 2)) and ref.ownedFreqs == [0, 1, 2]
ok = True
for lin, par in (('full', 'joint'), ('full', 'c'), ('operator', 'c')):
    v, p, r = inputs(prob, sv, par)
    kw = dict(linearisation=lin, parameter=par)
    F = prob.fieldsDevice()
    assert F.ownedFreqs == prob.ownedFreqs
    e = [ac.rel(prob.Jtvec(None, r, u=F, adjoint='transpose', **kw), ref.Jtvec(None, r, adjoint='transpose', **kw)),
         ac.rel(prob.JvecBorn(None, v, u=F, **kw), ref.JvecBorn(None, v, **kw)),
         ac.rel(prob.Hvec(None, p, **kw), ref.Hvec(None, p, **kw)),
         ac.rel(sv.dpred(u=F), sref.dpred())]
    F.release()
    print('RANK', dist.get_rank(), lin, par, ['%%.2e' %% x for x in e], flush=True)
    ok = ok and max(e) <= 1e-12
print('RANK', dist.get_rank(), 'OK' if ok else 'FAIL', flush=True)
dist.barrier(); dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_gloo_ranks_give_the_single_rank_result_on_the_device(helm_lib, tmp_path):
    """the three frequencies -- three grids -- sharded over two ranks on one GPU: every rank's store holds its own grids, its transposed transfers land on the
    native grid, and the all-reduce of the native-grid vector (of the data for JvecBorn) gives every rank the single-rank result"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'ranks.py'
    script.write_text(RANKS % dict(root=root))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29663', WORLD_SIZE='2', PYTHONPATH=root)
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
