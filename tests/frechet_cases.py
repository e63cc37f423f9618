"""Shared by tests/test_frechet_host.py (CPU) and tests/test_gpu_frechet.py (GPU): the survey the exact Frechet derivative (linearisation='operator')
is tested on, the Taylor and Richardson loops, and the 80-bit evaluation of the two device kernels with the componentwise bound they are held to."""
import numpy as np

from tests import adjoint_cases as ac
import zephyr_amd as za
from zephyr_amd.problem import Helm2DProblem, MZ_MASS
from zephyr_amd.survey import Helm2DSurvey

NZ, NX, NPML, DX = 37, 53, 6, 12.5
# three frequencies, the last one damped: a finite tau for ONE frequency is the complex frequency with the same omega_d = 2 pi f - i / tau (tau = 0.4 s)
FREQS = (5., 7., 9. - 1j / (2 * np.pi * 0.4))
NSRC, NREC = 5, 7
TAYLOR_H = (1., 0.5, 0.25, 0.125)


def model(seed=11):
    'c random in 2000 .. 2600, an explicit rough rho in 1800 .. 2300'
    rng = np.random.default_rng(seed)
    return rng.uniform(2000., 2600., (NZ, NX)), rng.uniform(1800., 2300., (NZ, NX))


def perturbation(seed=12, amplitude=50.):
    """v random with amplitude 50, zero in the absorbing layers and on the boundary.  The top is a free surface, but its nPML rows are stretched all the
    same (a free surface drops only the sign of the profile's first-derivative term), so they are zeroed too"""
    rng = np.random.default_rng(seed)
    v = amplitude * rng.uniform(-1., 1., (NZ, NX))
    v[:NPML, :] = 0.
    v[-NPML:, :] = 0.
    v[:, :NPML] = 0.
    v[:, -NPML:] = 0.
    return v.ravel()


def config(mode, hd, **extra):
    rng = np.random.default_rng(3)
    c, rho = model()
    X, Z = DX * (NX - 1), DX * (NZ - 1)
    lo = NPML + 3
    src = np.stack([np.linspace(DX * lo, X - DX * lo, NSRC), np.full(NSRC, DX * 4.3)], axis=1)
    if mode == 'fixed':
        rec = np.stack([np.linspace(DX * (lo + 0.4), X - DX * (lo + 0.6), NREC), np.full(NREC, Z - DX * (lo + 0.7))], axis=1)
    else:
        rec = np.stack([np.linspace(-2.3 * DX, 2.1 * DX, NREC), np.full(NREC, DX * 14.2)], axis=1)
    geom = dict(src=src, rec=rec, mode=mode, sterms=ac.randc(rng, NSRC), rterms=ac.randc(rng, NREC))
    sc = dict(nx=NX, nz=NZ, dx=DX, dz=DX, c=c, rho=rho, nPML=NPML, freeSurf=(True, False, False, False), freqs=list(FREQS),
              sterms=ac.randc(rng, len(FREQS)), geom=geom, parallel=False)
    if hd:
        sc.update(scaleTerm=0.7 - 0.2j)
    sc.update(extra)
    return sc


def host_pair(mode='fixed', hd=False, **extra):
    'the 37 x 53 case on the oracle doubles, numpy routes forced'
    sc = config(mode, hd, Disc=ac.OracleMiniZephyrHDT if hd else ac.OracleMiniZephyrT, hostGradient=True, **extra)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def device_pair(mode='fixed', hd=False, **extra):
    'the same case on the GPU operators'
    sc = config(mode, hd, Disc=za.MiniZephyrHD if hd else za.MiniZephyr, **extra)
    prob, sv = Helm2DProblem(sc), Helm2DSurvey(sc)
    prob.pair(sv)
    return prob, sv


def norm(a):
    return float(np.linalg.norm(np.asarray(a).ravel()))


def taylor_remainders(dpred, Jv, c0, v, hs=TAYLOR_H):
    '||d(c0 + h v) - d(c0) - h Jv|| for h in hs; dpred(c) -> data'
    d0 = dpred(c0)
    return [norm(dpred(c0 + h * v.reshape(c0.shape)) - d0 - h * Jv) for h in hs]


def factors(r):
    return [r[i] / r[i + 1] for i in range(len(r) - 1)]


def central(f, c0, v, h):
    '(f(c0 + h v) - f(c0 - h v)) / 2h'
    dv = v.reshape(c0.shape)
    return (f(c0 + h * dv) - f(c0 - h * dv)) / (2 * h)


# ---- the two kernels in 80-bit arithmetic -----------------------------------------------------------------------------------------------------
LD = np.longdouble
CLD = np.clongdouble
U64 = 2.0 ** -53
# roundings per component the kernels' operation order allows, counted generously from the code:
#   one term  w * u  (complex product, a component = two products and a sum)        <= 3
#   the nine-term sum: centre product, 4-sum of edges, 4-sum of corners, two weight products and two joins   <= 3 + 1 + 1 + 1 = 6 per term at most
#   the product with coef (virtual sources) or with uF_s and then W (imaging), a component = two products and a sum each    <= 3, twice for imaging
#   the sum over s and the final accumulation into G (imaging)     <= nsrc + 1
C_VIRTUAL = 3 + 6 + 3
def c_imaging(nsrc):
    return 6 + 3 + 3 + nsrc + 1


def _interior(nz, nx):
    m = np.zeros((nz, nx), dtype=bool)
    m[1:-1, 1:-1] = True
    return m


def _stencil(a, nz, nx, weights, absolute=False):
    'sum_k m_k a(i + k) over the nine neighbours inside the grid, in longdouble; a: (nz, nx) of any longdouble kind'
    p = np.zeros((nz + 2, nx + 2), dtype=a.dtype)
    p[1:-1, 1:-1] = a
    mc, md, me = [LD(w) for w in weights]
    sh = lambda dz, dx: p[1 + dz:1 + dz + nz, 1 + dx:1 + dx + nx]
    return mc * a + md * (sh(-1, 0) + sh(1, 0) + sh(0, -1) + sh(0, 1)) + me * (sh(-1, -1) + sh(-1, 1) + sh(1, -1) + sh(1, 1))


def _absprod(a, b):
    '|Re a||Re b| + |Im a||Im b| + |Re a||Im b| + |Im a||Re b| halves: the magnitude that bounds either component of a b'
    return np.maximum(np.abs(a.real) * np.abs(b.real) + np.abs(a.imag) * np.abs(b.imag), np.abs(a.real) * np.abs(b.imag) + np.abs(a.imag) * np.abs(b.real))


def virtual_sources_reference(U, W, coef, nz, nx, conj, weights=MZ_MASS, mask=True, dtype=CLD):
    """R[s] = coef mask_int (.) M0(W (.) conj-or-not(U[s])) and the magnitude sum_k m_k (|Re W||Re u| + |Im W||Im u|) |coef| per cell the bound scales.
    U (nsrc, N), W (N,).  dtype CLD: the 80-bit evaluation; np.complex128: the plain fp64 one."""
    real = LD if dtype is CLD else np.float64
    Ux = np.asarray(U).astype(dtype)
    Wx = np.asarray(W).astype(dtype)
    if conj:
        Ux = np.conj(Ux)
    cf = dtype(coef)
    inside = _interior(nz, nx)
    out = np.zeros(Ux.shape, dtype=dtype)
    mag = np.zeros(Ux.shape, dtype=real)
    acoef = abs(cf.real) + abs(cf.imag)
    for s in range(Ux.shape[0]):
        t = (Wx * Ux[s]).reshape(nz, nx)
        r = cf * _stencil(t, nz, nx, weights)
        m = acoef * _stencil(_absprod(Wx, Ux[s]).astype(real).reshape(nz, nx), nz, nx, weights)
        if mask:
            r = np.where(inside, r, 0)
            m = np.where(inside, m, 0)
        out[s], mag[s] = r.ravel(), m.ravel()
    return out, mag


def imaging_reference(G0, UF, UB, W, nz, nx, weights=MZ_MASS, mask=True, dtype=CLD):
    """G = G0 + W (.) sum_s UF[s] (.) M0(mask_int (.) UB[s]) and the magnitude |G0| + (|Re W| + |Im W|) sum_s sum_k m_k(...) the bound scales"""
    real = LD if dtype is CLD else np.float64
    F = np.asarray(UF).astype(dtype)
    B = np.asarray(UB).astype(dtype)
    Wx = np.asarray(W).astype(dtype)
    inside = _interior(nz, nx)
    acc = np.zeros(F.shape[1], dtype=dtype)
    mag = np.zeros(F.shape[1], dtype=real)
    for s in range(F.shape[0]):
        b = B[s].reshape(nz, nx)
        ab = (np.abs(b.real) + np.abs(b.imag)).astype(real)
        if mask:
            b = np.where(inside, b, 0)
            ab = np.where(inside, ab, 0)
        acc = acc + F[s] * _stencil(b, nz, nx, weights).ravel()
        mag = mag + (np.abs(F[s].real) + np.abs(F[s].imag)) * _stencil(ab, nz, nx, weights).ravel()
    aw = np.abs(Wx.real) + np.abs(Wx.imag)
    g0 = np.asarray(G0).astype(dtype)
    return g0 + Wx * acc, np.abs(g0.real) + np.abs(g0.imag) + aw * mag


def worst_ratio(got, ref, bound):
    'max over components of |got - ref| / bound (0 / 0 counts as 0: a cell the mask zeroes must be exactly zero)'
    got = np.asarray(got).astype(CLD)
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max())


def kernel_inputs(nz, nx, nsrc, seed=0):
    rng = np.random.default_rng(seed)
    N = nz * nx
    U = ac.randc(rng, (nsrc, N)) * 10.0 ** rng.uniform(-3, 3, (nsrc, 1))
    B = ac.randc(rng, (nsrc, N))
    W = ac.randc(rng, N)
    G0 = ac.randc(rng, N)
    return U, B, W, G0
