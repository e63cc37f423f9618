"""CPU: linearisation='full' of JvecBorn / Jtvec / Hvec on the oracle doubles -- the velocity planes (mass term, PML stretch, Gardner chain) against the oracle's
own assembly by a Taylor test that the mass term alone fails, their transpose, the Taylor test of dpred with a perturbation that is non-zero in the absorbing
layers (which 'operator' fails), the adjoint identities, the refusals, and the 80-bit evaluations the two device kernels are held to."""
import numpy as np
import pytest

import zephyr_amd as za
from oracle import helm_oracle as ho
from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from zephyr_amd import frechet as fr

CASES = [('fixed', False), ('fixed', True), ('relative', False), ('relative', True)]
IDS = ['fixed-mz', 'fixed-hd', 'moving-mz', 'moving-hd']
FULL = dict(linearisation='full')
OP = dict(linearisation='operator')
SECOND, FIRST = 3.5, 2.5          # the windows of the Taylor tests of test_frechet_host.py / test_density_host.py: factors >= 3.5 second order, <= 2.5 first order


@pytest.fixture(scope='module')
def solved():
    'per case and density (explicit, Gardner): the pair, the velocity of the config, the perturbation, the host fields and the Born data -- made once'
    out = {}
    for key in CASES:
        for density in (True, False):
            prob, sv = xc.pair(*key, density=density)
            c0 = np.array(prob.systemConfig['c'], dtype=np.float64)
            v = xc.perturbation()
            uF = prob.fields()
            out[key + (density,)] = dict(prob=prob, sv=sv, c0=c0, v=v, uF=uF, Jv=prob.JvecBorn(None, v, u=uF, **FULL))
    return out


# ---- 1. the velocity planes against the oracle's assembly ----------------------------------------------------------------------------------------
def _oracle_planes(sc, c, rho):
    return ho.minizephyr_coefficients(sc['nz'], sc['nx'], c, rho, complex(sc['freq']), dx=sc['dx'], dz=sc['dz'], nPML=sc['nPML'], tau=sc.get('tau', np.inf),
                                      ky=sc.get('ky', 0.0), freeSurf=sc['freeSurf'])


@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_taylor_remainder_of_the_planes_falls_at_second_order_and_the_mass_term_alone_does_not(name, density):
    """||A(c + h dc) - A(c) - h dA||_inf over the interior rows of the oracle's nine planes, dc non-zero in every cell: second order with velocityPlanes, first
    order with the mass term alone (what 'operator' applies) and, where the density follows c, with mass term and stretch but no Gardner chain."""
    sc = xc.operator_config(name, density)
    op = za.MiniZephyr(sc)
    nz, nx = sc['nz'], sc['nx']
    v, _, _, _ = xc.operator_inputs(sc)
    c0 = np.asarray(sc['c'], dtype=np.float64)
    rho = (lambda c: sc['rho']) if density else (lambda c: 310. * c ** 0.25)
    db = None if density else fr.gardnerChain(c0) * v
    inside = fr._interiorMask(nz, nx)
    A0 = _oracle_planes(sc, c0, rho(c0))
    candidates = {'full': fr.velocityPlanes(op, v, db), 'mass': xc.mass_only_planes(op, v)}
    if not density:
        candidates['no chain'] = fr.velocityPlanes(op, v)
    assert np.all(candidates['full'][:, ~inside] == 0)
    rem = {k: [] for k in candidates}
    for h in fc.TAYLOR_H:
        c1 = c0 + h * v.reshape((nz, nx))
        D = _oracle_planes(sc, c1, rho(c1)) - A0
        D[:, ~inside] = 0
        for k, dA in candidates.items():
            rem[k].append(float(np.abs(D - h * dA).max()))
    print('%s %s: %s' % (name, 'rho' if density else 'gardner', {k: ['%.2f' % f for f in fc.factors(r)] for k, r in rem.items()}))
    assert all(f >= SECOND for f in fc.factors(rem['full']))
    for k in candidates:
        if k != 'full':
            assert all(f <= FIRST for f in fc.factors(rem[k])), k


@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_velocity_adjoint_is_the_plain_transpose(name):
    "<V[dc], P> = <dc, V^T P> under the bilinear pairing for random complex P, to rounding; the same conjugated, and with the Gardner chain joined"
    sc = xc.operator_config(name)
    op = za.MiniZephyr(sc)
    _, _, P, _ = xc.operator_inputs(sc)
    x = np.random.default_rng(2).standard_normal(P.shape[1])
    V = fr.velocityPlanes(op, x).reshape((9, -1))
    for conj in (False, True):
        Vc = np.conj(V) if conj else V
        lhs, rhs = (Vc * P).sum(), (x * fr.velocityAdjoint(op, P, conj=conj)).sum()
        scale = (np.abs(V) * np.abs(P)).sum()
        assert abs(lhs - rhs) <= 64 * dc.U64 * scale, (name, conj, abs(lhs - rhs) / scale)
    chain = fr.gardnerChain(sc['c'])
    T = fr.velocityPlanes(op, x, chain * x).reshape((9, -1))
    lhs, rhs = (T * P).sum(), (x * (fr.velocityAdjoint(op, P) + chain * fr.buoyancyAdjoint(op, P))).sum()
    assert abs(lhs - rhs) <= 64 * dc.U64 * ((np.abs(V) + np.abs(T - V)) * np.abs(P)).sum()
    # linear in dc
    y = np.random.default_rng(4).standard_normal(x.size)
    assert np.abs(fr.velocityPlanes(op, x) + fr.velocityPlanes(op, y) - fr.velocityPlanes(op, x + y)).max() <= 16 * dc.U64 * fr.velocityPlanes(op, np.abs(x) + np.abs(y), magnitude=True).max()


def test_gardner_chain_is_the_derivative_of_the_default_buoyancy():
    c = np.linspace(1500., 4500., 13)
    b = lambda x: 1.0 / (310. * x ** 0.25)
    fd = (b(c + 1e-3) - b(c - 1e-3)) / 2e-3
    assert np.abs(fr.gardnerChain(c) - fd).max() <= 1e-9 * np.abs(fd).max()
    assert np.array_equal(fr.gardnerChain(c * (1 + 0.02j)), fr.gardnerChain(c))          # (the density follows Re(c))


# ---- 2. Taylor at the level of dpred ----------------------------------------------------------------------------------------------------------------
# The h ladder is frechet_cases.TAYLOR_H with the perturbation of density_cases (+-50, non-zero everywhere) as it is: at h = 1 every case, the Gardner ones
# included, is in the asymptotic range already (factors 3.97 .. 4.00), so the amplitude is not shrunk.
@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_taylor_remainder_of_dpred_falls_at_second_order(solved, key, density):
    s = solved[key + (density,)]
    r = xc.taylor_remainders(s['prob'], s['sv'], s['Jv'], s['c0'], s['v'])
    print('%s %s: remainders %s factors %s' % (key, density, r, fc.factors(r)))
    assert all(f >= SECOND for f in fc.factors(r))


@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_operator_is_of_first_order_on_the_same_perturbation_and_equal_where_it_vanishes_in_the_layers(solved, key):
    """the gap 'full' closes: with the perturbation non-zero in the absorbing layers the remainder of 'operator' heads for first order -- its factors fall from
    step to step, leave the second-order window and end inside the first-order one (at h = 1 the common h^2 term still weighs in) -- while with the in-layer-zero
    perturbation of frechet_cases the two are the same to rounding"""
    s = solved[key + (True,)]
    prob, sv, uF, v = s['prob'], s['sv'], s['uF'], s['v']
    Jop = prob.JvecBorn(None, v, u=uF, **OP)
    f = fc.factors(xc.taylor_remainders(prob, sv, Jop, s['c0'], v))
    print('%s: operator factors %s' % (key, f))
    assert f[0] > f[1] > f[2] and f[2] <= FIRST and min(f) < SECOND
    v0 = fc.perturbation()
    assert ac.rel(prob.JvecBorn(None, v0, u=uF, **FULL), prob.JvecBorn(None, v0, u=uF, **OP)) <= 1e-12
    r = ac.randc(np.random.default_rng(3), sv.nD)
    gf, go = prob.Jtvec(None, r, u=uF, adjoint='transpose', **FULL), prob.Jtvec(None, r, u=uF, adjoint='transpose', **OP)
    interior = v0 != 0
    assert ac.rel(gf[interior], go[interior]) <= 1e-12 and ac.rel(gf, go) > 1e-3          # (the gradients differ in the layers, and only there)


# ---- 3. the adjoint identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('density', [True, False], ids=['rho', 'gardner'])
@pytest.mark.parametrize('key', CASES, ids=IDS)
def test_full_pair_is_adjoint_and_hvec_is_symmetric(solved, key, density):
    "the tolerance 1e-10 is that of the 'operator' identity of test_frechet_host.py / test_density_host.py"
    s = solved[key + (density,)]
    prob, sv, uF = s['prob'], s['sv'], s['uF']
    rng = np.random.default_rng(17)
    x, y, r = rng.standard_normal(prob.nrow), rng.standard_normal(prob.nrow), ac.randc(rng, sv.nD)
    Jx = prob.JvecBorn(None, x, u=uF, **FULL)
    g = prob.Jtvec(None, r, u=uF, adjoint='transpose', **FULL)
    assert g.shape == (prob.nrow,) and g.dtype == np.float64 and Jx.dtype == np.complex128 and Jx.shape == (sv.nD,)
    lhs = ac.inner(Jx, r)
    miss = abs(lhs - ac.inner(x, g)) / abs(lhs)
    print('%s %s: identity misses by %.2e' % (key, density, miss))
    assert miss <= 1e-10
    H = lambda p: prob.Hvec(None, p, u=uF, **FULL)
    a, b = float(x @ H(y)), float(y @ H(x))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
    assert abs(float(x @ H(x)) - ac.inner(Jx, Jx)) <= 1e-10 * ac.inner(Jx, Jx)
    # u = None solves the fields itself and gives the same
    assert ac.rel(prob.JvecBorn(None, x, **FULL), Jx) <= 1e-12
    assert ac.rel(prob.Jtvec(None, r, adjoint='transpose', **FULL), g) <= 1e-12
    if density:
        # parameter='rho' with 'full' is 'operator' under another name, and the blocks of Hvec take 'full' in both halves
        kw = dict(u=uF, parameter='rho')
        assert np.array_equal(prob.JvecBorn(None, x, **kw, **FULL), prob.JvecBorn(None, x, **kw, **OP))
        assert np.array_equal(prob.Jtvec(None, r, adjoint='transpose', **kw, **FULL), prob.Jtvec(None, r, adjoint='transpose', **kw, **OP))
        a, b = float(y @ prob.Hvec(None, x, u=uF, parameter=('c', 'rho'), **FULL)), float(x @ prob.Hvec(None, y, u=uF, parameter=('rho', 'c'), **FULL))
        assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
        assert abs(a - ac.inner(Jx, prob.JvecBorn(None, y, **kw, **OP))) <= 1e-10 * abs(a)


# ---- 4. the refusals ---------------------------------------------------------------------------------------------------------------------------------
def _all_three_refuse(prob, sv, **kw):
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for call in (lambda: prob.JvecBorn(None, v, **kw), lambda: prob.Jtvec(None, r, adjoint='transpose', **kw), lambda: prob.Hvec(None, v, **kw)):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert len(str(ei.value)) > 20
    return str(ei.value)


def test_what_full_does_not_serve_is_refused_with_the_messages_of_operator():
    from zephyr_amd import MiniZephyr, MultiGridMultiFreq
    from zephyr_amd.problem import Helm2DProblem, Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey, Helm2DMultiGridSurvey
    from tests.test_moving_plan import multigrid_config
    prob25, sv25 = ac.host_pair('25d-fixed', rho=2000.)
    scv = fc.config('fixed', False, Disc=ac.OracleMiniZephyrT, hostGradient=True, Q=50.)
    probv, svv = Helm2DViscoProblem(scv), Helm2DSurvey(scv)
    probv.pair(svv)
    sce = fc.config('fixed', False, Disc=za.Eurus, hostGradient=True)
    probe, sve = Helm2DProblem(sce), Helm2DSurvey(sce)
    probe.pair(sve)
    scm = dict(multigrid_config(), Disc=MiniZephyr, SystemWrapper=MultiGridMultiFreq, rho=2000.)
    probm, svm = Helm2DProblem(scm), Helm2DMultiGridSurvey(scm)
    probm.pair(svm)
    for prob, sv in ((prob25, sv25), (probv, svv), (probe, sve), (probm, svm)):
        full = _all_three_refuse(prob, sv, **FULL)
        assert full.replace("'full'", "'operator'") == _all_three_refuse(prob, sv, **OP)


def test_full_without_rho_refuses_the_density_and_operator_still_refuses_the_config(solved):
    s = solved[('fixed', False, False)]
    prob, sv = s['prob'], s['sv']
    assert 'free parameter' in _all_three_refuse(prob, sv, parameter='rho', **FULL)
    with pytest.raises(NotImplementedError, match='free parameter'):
        prob.Hvec(None, np.ones(prob.nrow), parameter=('c', 'rho'), **FULL)
    assert 'rho' in _all_three_refuse(prob, sv, **OP)                      # ('operator' without `rho`: as before)
    r, v = np.ones(sv.nD, dtype=complex), np.ones(prob.nrow)
    for call in (lambda: prob.JvecBorn(None, v, linearisation='total'), lambda: prob.Jtvec(None, r, u=s['uF'], **FULL),          # (adjoint='reciprocity')
                 lambda: prob.Hvec(None, v, parameter='Q', **FULL)):
        with pytest.raises(ValueError):
            call()


# ---- 5. the reference evaluations of the two kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(dc.OPERATOR_CASES))
def test_the_80_bit_velocity_map_and_transpose_bound_plain_fp64_and_reject_wrong_ones(name):
    sc = xc.operator_config(name)
    op = za.MiniZephyr(sc)
    v, db, P, G0 = xc.operator_inputs(sc)
    N = v.size
    worst = []
    for d, c in ((None, xc.C_VPLANES), (db, xc.C_VPLANES_DB)):
        ref, mag = xc.planes_reference(op, v, d)
        bound = c * xc.U64 * mag
        plain = fr.velocityPlanes(op, v, d).reshape((9, N))
        worst.append(xc.worst_ratio(plain, ref, bound))
        assert worst[-1] <= 1.0
        assert xc.worst_ratio(plain[::-1], ref, bound) > 1e6                        # (the planes in the wrong slots)
    ref, mag = xc.planes_reference(op, v)
    assert xc.worst_ratio(xc.planes_without_x_over_den(op, v).reshape((9, N)), ref, xc.C_VPLANES * xc.U64 * mag) > 1e6
    assert xc.worst_ratio(xc.mass_only_planes(op, v).reshape((9, N)), ref, xc.C_VPLANES * xc.U64 * mag) > 1e6
    w = -0.7 + 0.4j
    for conj in (False, True):
        ref, mag = xc.adjoint_reference(op, G0, P, w, conj)
        bound = xc.C_VADJOINT * xc.U64 * mag
        worst.append(xc.worst_ratio(G0 + w * fr.velocityAdjoint(op, P, conj=conj), ref, bound))
        assert worst[-1] <= 1.0
        assert xc.worst_ratio(G0 + w * fr.velocityAdjoint(op, P, conj=not conj), ref, bound) > 1e6
    print('%s: fp64 numpy at %s of the bounds' % (name, ['%.3f' % x for x in worst]))
