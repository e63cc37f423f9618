"""Shared by tests/test_visco_host.py (CPU) and tests/test_gpu_visco.py (GPU): the exact velocity and Q derivatives of a visco problem (parameter 'c', 'Q', 'cQ'
of JvecBorn / Jtvec / Hvec on a Helm2DViscoProblem) on the 37 x 53 survey of tests/frechet_cases.py, and the 80-bit evaluations of the three device kernels with
the componentwise bounds they are held to.

The bounds, in the style of tests/density_cases.py and tests/full_cases.py: c u m per component, u = 2^-53, m the `magnitude` evaluation, c a count of roundings
read off the kernels' operation order (csrc/survey_visco.hip), generously:

  the chain (visco_chain)   q = 1 / Q (1); disp = 1 + lam q (a product and a sum on top of q: 3), att = 1 + i q / 2 (q's own: 1); gamma = disp att (1 more): 5.
                            chi: the Smith division (i / 2) / att (6 on top of 1: 7), the dispersion term lam / disp (4) and the join (1): 8; q^2 (2 from q and
                            a product: 3) and its product with the bracket (1): 12; the complex product with c~ (3; c~ is the handle's, an exact input): 15;
                            the sign is exact.  One to spare.                                                                          C_CHAIN = 16
  k_visco_perturbation      gamma v_c (1 more) and chi v_Q (1 more), one complex multiply-add joining them (2).                       C_PERTURB = C_CHAIN + 4
  k_visco_chain_adjoint     the product with T (3 on top of the chain) and the addition into G (1).                                   C_CHAINADJ = C_CHAIN + 4
  k_velocity_planes_z       k_velocity_planes (full_cases.C_VPLANES = 68) with complex products where it has real scalings: a differentiated row factor times
                            dc~_i (3 instead of 1) and (d kappa / dc) b times dc~_j (3 instead of 1).                                  C_VPLANES_Z = 68 + 4
"""
import numpy as np

from tests import adjoint_cases as ac
from tests import density_cases as dc
from tests import frechet_cases as fc
from tests import full_cases as xc
from zephyr_amd import frechet as fr

LD, CLD, U64 = fc.LD, fc.CLD, fc.U64
C_CHAIN = 16
C_PERTURB = C_CHAIN + 4
C_CHAINADJ = C_CHAIN + 4
C_VPLANES_Z = xc.C_VPLANES + 4

STRONG_H = (1., 0.5, 0.25, 0.125, 0.0625, 0.03125)          # the six steps: with fewer the derivative without the chain cannot be told from the right one
SECOND = 3.9                                                 # every factor of a Taylor remainder of the right derivative (measured on the host: 4.00 .. 4.15)
FIRST = 3.0                                                  # some factor of a wrong one falls below this (measured: 2.0 .. 2.5)
PARAMETERS = ('c', 'Q', 'cQ')


def strong_config(mode='fixed', hd=False, device=False, **extra):
    'the 37 x 53 case with strong attenuation and dispersion: Q uniform in 8 .. 40, freqBase 6, real frequencies 5, 7, 9 with tau = 0.4'
    import zephyr_amd as za
    Q = np.random.default_rng(5).uniform(8., 40., (fc.NZ, fc.NX))
    if device:
        cls = dict(Disc=za.MiniZephyrHD if hd else za.MiniZephyr)
    else:
        cls = dict(Disc=ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT, hostGradient=True)
    sc = fc.config(mode, hd, Q=Q, freqBase=6., tau=0.4, viscoDerivatives=True, **cls)
    sc['freqs'] = [5., 7., 9.]
    sc.update(extra)
    return sc


def weak_config(mode='relative', hd=True, device=False, **extra):
    'the second case: a complex frequency (fc.FREQS) and no dispersion (freqBase 0), Q uniform in 30 .. 120'
    import zephyr_amd as za
    Q = np.random.default_rng(5).uniform(30., 120., (fc.NZ, fc.NX))
    if device:
        cls = dict(Disc=za.MiniZephyrHD if hd else za.MiniZephyr)
    else:
        cls = dict(Disc=ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT, hostGradient=True)
    sc = fc.config(mode, hd, Q=Q, freqBase=0., viscoDerivatives=True, **cls)
    sc.update(extra)
    return sc


def pair(sc, Problem=None):
    from zephyr_amd.problem import Helm2DViscoProblem
    from zephyr_amd.survey import Helm2DSurvey
    prob, sv = (Problem or Helm2DViscoProblem)(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def perturbations(layers=True):
    """(v_c, v_Q): +-50 in c and +-2 in Q.  layers: non-zero everywhere, boundary lines and absorbing layers included (what 'full' is exact for);
    otherwise zero in the layers (what 'operator' is exact for)"""
    if layers:
        return dc.perturbation(seed=31), dc.perturbation(seed=32, amplitude=2.)
    return fc.perturbation(seed=31), fc.perturbation(seed=32, amplitude=2.)


def stacked(parameter, vc, vQ):
    "the perturbation vector of a parameter: v_c, v_Q or [v_c; v_Q]"
    return {'c': vc, 'Q': vQ, 'cQ': np.concatenate([vc, vQ])}[parameter]


def halves(parameter, vc, vQ):
    "(dc, dQ) a parameter moves the model along"
    return (vc if parameter in ('c', 'cQ') else 0. * vc), (vQ if parameter in ('Q', 'cQ') else 0. * vQ)


def taylor_remainders(prob, sv, Jv, parameter, vc, vQ, hs=STRONG_H, dpred=None):
    '||d(c + h dc, Q + h dQ) - d(c, Q) - h Jv|| for h in hs; the model is put back.  dpred: model dict -> data (default sv.dpred)'
    dpred = sv.dpred if dpred is None else dpred
    shape = (fc.NZ, fc.NX)
    c0 = np.array(prob.systemConfig['c'], dtype=np.float64).reshape(shape)
    Q0 = np.array(prob.systemConfig['Q'], dtype=np.float64).reshape(shape)
    dcv, dQv = halves(parameter, vc, vQ)
    at = lambda h: {'c': c0 + h * dcv.reshape(shape), 'Q': Q0 + h * dQv.reshape(shape)}
    d0 = dpred(at(0.))
    out = [fc.norm(dpred(at(h)) - d0 - h * Jv) for h in hs]
    prob.updateModel(at(0.))
    return out


def chainless_born(prob, sv, uF, parameter, vc, vQ):
    """the Born data with the chain left out -- gamma = 1 and chi replaced by its real part, a REAL perturbation of the complex velocity -- through the host
    route of density_cases.born_with_planes: a wrong derivative"""
    dcv, dQv = halves(parameter, vc, vQ)
    lam = {id(op): prob._viscoLambda(i) for i, op in enumerate(prob.system.subProblems)}

    def planes(op):
        _, chi = fr.viscoChain(prob.systemConfig['c'], prob._viscoQ(), lam[id(op)])
        return fr.velocityPlanes(op, dcv + chi.real * dQv)
    return dc.born_with_planes(prob, sv, uF, planes)


# ---- the three kernels in 80-bit arithmetic -----------------------------------------------------------------------------------------------------------
def kernel_model(sc, seed=9):
    "(c real, Q) of a handle's grid: Q rough in 8 .. 40 with every seventh cell infinite"
    rng = np.random.default_rng(seed)
    N = sc['nz'] * sc['nx']
    Q = rng.uniform(8., 40., N)
    Q[::7] = np.inf
    return np.asarray(sc['c'], dtype=np.float64).ravel(), Q


def complex_velocity(c, Q, lam):
    "c~ as ViscoMultiFreq.spUpdates makes it, in its own operation order (what a handle's d_c holds)"
    c, Q = np.asarray(c, dtype=np.float64).ravel(), np.asarray(Q, dtype=np.float64).ravel()
    cR = (1. + lam / Q) * c if lam != 0. else c
    return cR + (0.5j * cR / Q)


def chain_reference(ct, Q, lam, dispersion=True):
    """(gamma, chi) and their magnitudes in 80-bit arithmetic from the complex velocity ct the handle holds, as the kernels take them: chi = -ct q^2 [...].
    dispersion False: chi without its dispersion term (a wrong evaluation when lam != 0)"""
    q = 1 / np.asarray(Q, dtype=np.float64).astype(LD)
    lamx, half = LD(lam), CLD(0.5j)
    disp, att = 1 + lamx * q, 1 + half * q
    gamma = disp * att
    ctx = np.asarray(ct).astype(CLD)
    bracket = (lamx / disp if dispersion else 0) + half / att
    chi = -ctx * (q * q) * bracket
    gmag = (1 + abs(lamx) * q) * (1 + q / 2)
    cmag = (np.abs(ctx.real) + np.abs(ctx.imag)) * (q * q) * (abs(lamx) / np.abs(disp) + LD(0.5) * (1 + q / 2) / (np.abs(att) ** 2))
    return gamma, chi, gmag, cmag


def perturbation_reference(ct, Q, lam, vc, vQ, dispersion=True):
    'dc~ = gamma v_c + chi v_Q (either may be None) in 80-bit arithmetic, and the magnitude |gamma||v_c| + |chi||v_Q|'
    gamma, chi, gmag, cmag = chain_reference(ct, Q, lam, dispersion)
    ref, mag = np.zeros(gamma.shape, dtype=CLD), np.zeros(gamma.shape, dtype=LD)
    if vc is not None:
        ref, mag = ref + gamma * np.asarray(vc).astype(LD), mag + gmag * np.abs(np.asarray(vc).astype(LD))
    if vQ is not None:
        ref, mag = ref + chi * np.asarray(vQ).astype(LD), mag + cmag * np.abs(np.asarray(vQ).astype(LD))
    return ref, mag


def chain_adjoint_reference(ct, Q, lam, T, G0, conj, dispersion=True):
    '(G0_c + gamma` T, G0_Q + chi` T) and the magnitudes, 80-bit; conj: the conjugated chain'
    gamma, chi, gmag, cmag = chain_reference(ct, Q, lam, dispersion)
    if conj:
        gamma, chi = np.conj(gamma), np.conj(chi)
    Tx = np.asarray(T).astype(CLD)
    at = np.abs(Tx.real) + np.abs(Tx.imag)
    out = []
    for g0, f, fm in ((G0[0], gamma, gmag), (G0[1], chi, cmag)):
        g0x = np.asarray(g0).astype(CLD)
        out.append((g0x + f * Tx, np.abs(g0x.real) + np.abs(g0x.imag) + fm * at))
    return out


def planes_z_reference(op, dcz):
    'V[dc~] for a complex perturbation in 80-bit arithmetic and the magnitude the bound scales: (9, N) each'
    N = int(op.nz) * int(op.nx)
    return fr.velocityPlanes(op, dcz, dtype=CLD).reshape((9, N)), fr.velocityPlanes(op, dcz, dtype=CLD, magnitude=True).reshape((9, N))


worst_ratio = fc.worst_ratio
