"""Shared by tests/test_ky_exact_host.py (CPU) and tests/test_gpu_ky_exact.py (GPU): the exact derivatives of a 2.5-D problem (kyDerivatives=True) -- the
24 x 20 survey of adjoint_cases on the oracle doubles and the 37 x 53 survey of frechet_cases on the GPU operators, both with nky = 3 (the quadrature weights
1/5, 2/5, 2/5 and three distinct ky) and an explicit cmin, and the gradient formed from the ky-SUMMED fields that the per-ky routes replace."""
import numpy as np

from tests import adjoint_cases as ac
from tests import frechet_cases as fc
import zephyr_amd as za
from zephyr_amd import frechet as fr
from zephyr_amd.problem import Helm2DProblem, Helm25DProblem
from zephyr_amd.survey import Helm2DSurvey, Helm25DSurvey

NKY = 3
CMIN = 2000.
HOST_NZ, HOST_NX = 24, 20
TAYLOR_H = (1., 0.5, 0.25, 0.125, 0.0625, 0.03125)          # five halvings
SECOND, FIRST = 3.5, 2.5                                      # the windows of tests/test_full_host.py


class OracleMiniZephyr25DHDT(za.MiniZephyr25D):
    'the ky sum with the HD doubles (complex premul default; the quadrature weight of spUpdates replaces it per ky) as sub-problems'

    @property
    def Disc(self):
        return ac.OracleMiniZephyrHDT


def host_rho(seed=21):
    'an explicit rough density, 1800 .. 2300'
    return np.random.default_rng(seed).uniform(1800., 2300., (HOST_NZ, HOST_NX))


def host_config(mode='fixed', hd=False, density=True, nky=NKY, **extra):
    """the 24 x 20 survey of adjoint_cases.survey_config (3 sources, 5 receivers, 15 / 20 / 25 Hz) as a 2.5-D problem on the oracle doubles, numpy routes forced;
    the velocity is the real part of the rough model (the Taylor tests step it along real perturbations); hd: MiniZephyrHD doubles and a complex scaleTerm"""
    sc = ac.survey_config(HOST_NZ, HOST_NX, 3, 5, ac.HOST_FREQS, 'relative' if mode != 'fixed' else 'fixed')
    sc['c'] = np.array(sc['c'].real)
    sc.update(Disc=OracleMiniZephyr25DHDT if hd else ac.OracleMiniZephyr25DT, nky=nky, cmin=CMIN, kyOnDevice=False, hostGradient=True, kyDerivatives=True)
    if density:
        sc['rho'] = host_rho()
    if hd:
        sc['scaleTerm'] = 0.7 - 0.2j
    sc.update(extra)
    return sc


def host_pair(mode='fixed', hd=False, density=True, **extra):
    sc = host_config(mode, hd, density, **extra)
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def host_pair_2d(mode='fixed', hd=False, **extra):
    """the same config as a 2-D problem on the 2-D doubles (what nky = 1 is compared with).  The composite hands every ky operator its quadrature weight as
    `premul` (1 for nky = 1), which replaces the half-differentiation default of the HD class: the 2-D config says premul = 1 for the same operator."""
    sc = host_config(mode, hd, True, **extra)
    for key in ('nky', 'cmin', 'kyOnDevice', 'kyDerivatives'):
        sc.pop(key)
    sc['premul'] = 1.0
    sc['Disc'] = ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def perturbation(n, seed=8, amplitude=50.):
    'uniform in +-amplitude and non-zero in every cell (density_cases.perturbation on this grid): boundary lines and absorbing layers included'
    v = amplitude * np.random.default_rng(seed).uniform(-1., 1., n)
    v[np.abs(v) < 1.] = 1.
    return v


def taylor_remainders(dpred, d0, Jv, hs=TAYLOR_H):
    '||d(h) - d0 - h Jv|| for h in hs; dpred(h) -> data at the model stepped by h'
    return [fc.norm(dpred(h) - d0 - h * Jv) for h in hs]


def summed_field_gradient(prob, r, linearisation='full'):
    """What the maps give when they are fed the ky SUMS: per frequency the lag products of sum_k z_k against sum_k u^_k, transposed with the ky = 0 operator and
    the weight -conj(st).  This is NOT a route of the product: it is the shortcut the per-ky routes exist to avoid, and it misses the adjoint identity."""
    sv = prob.survey
    resid = np.asarray(r).reshape((sv.nrec, sv.nsrc, sv.nfreq))
    adj = prob.adjointSystem
    qb = [q.conj() for q in sv.getResidualSources(np.conj(resid))]
    FK = prob.fields(perKy=True)
    g = np.zeros(prob.nrow, dtype=np.complex128)
    for ifreq in range(sv.nfreq):
        st = prob._kyScale(ifreq)
        subs, asubs = prob.system.subProblems[ifreq].subProblems, adj.subProblems[ifreq].subProblems
        z = sum(np.conj(np.asarray(a * qb[ifreq])) for a in asubs)          # (sum_k A_k^-T premul_k R^H r)
        u = np.conj(FK[ifreq].sum(axis=0) / st)
        P = fr.lagProducts(z, u, subs[0].nz, subs[0].nx)
        g += -np.conj(st) * fr.velocityAdjoint(subs[0], P, stretch=linearisation == 'full')
    return g.real


# ---- the GPU case --------------------------------------------------------------------------------------------------------------------------------------
GPU_FREQS = (5., 7.)
GPU_NSRC, GPU_NREC = 3, 5


def device_config(mode='fixed', hd=False, density=True, **extra):
    """the 37 x 53 grid of frechet_cases (several separator levels) as a 2.5-D problem on the GPU operators: two frequencies, 3 sources, 5 receivers, nky = 3,
    real receiver terms (host_of() is the same survey on the oracle doubles)"""
    rng = np.random.default_rng(3)
    NZ, NX, NPML, DX = fc.NZ, fc.NX, fc.NPML, fc.DX
    c, rho = fc.model()
    X, Z = DX * (NX - 1), DX * (NZ - 1)
    lo = NPML + 3
    src = np.stack([np.linspace(DX * lo, X - DX * lo, GPU_NSRC), np.full(GPU_NSRC, DX * 4.3)], axis=1)
    if mode == 'fixed':
        rec = np.stack([np.linspace(DX * (lo + 0.4), X - DX * (lo + 0.6), GPU_NREC), np.full(GPU_NREC, Z - DX * (lo + 0.7))], axis=1)
    else:
        rec = np.stack([np.linspace(-2.3 * DX, 2.1 * DX, GPU_NREC), np.full(GPU_NREC, DX * 14.2)], axis=1)
    geom = dict(src=src, rec=rec, mode='fixed' if mode == 'fixed' else 'relative', sterms=ac.randc(rng, GPU_NSRC), rterms=np.abs(ac.randc(rng, GPU_NREC)) + 0.5)
    sc = dict(nx=NX, nz=NZ, dx=DX, dz=DX, c=c, nPML=NPML, freeSurf=(True, False, False, False), freqs=list(GPU_FREQS), sterms=ac.randc(rng, len(GPU_FREQS)),
              geom=geom, parallel=False, Disc=za.MiniZephyr25D, nky=NKY, cmin=CMIN, kyDerivatives=True, rtol=1e-11)
    if density:
        sc['rho'] = rho
    if hd:
        sc.update(scaleTerm=0.7 - 0.2j)
    sc.update(extra)
    return sc


def device_pair(mode='fixed', hd=False, density=True, **extra):
    sc = device_config(mode, hd, density, **extra)
    prob, sv = Helm25DProblem(sc), Helm25DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def host_of(mode='fixed', hd=False, density=True, **extra):
    'the oracle doubles on the survey of device_config, numpy routes forced: what the device routes are compared with, fed the downloaded per-ky blocks'
    return device_pair(mode, hd, density, Disc=ac.OracleMiniZephyr25DT, kyOnDevice=False, hostGradient=True, **extra)
