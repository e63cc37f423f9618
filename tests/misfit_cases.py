"""Shared by tests/test_misfit_host.py (CPU), tests/test_gpu_misfit.py, tests/test_gpu_misfit_routes.py and tests/test_gpu_misfit_onepass.py (GPU): the
kinds and their parameters, data-space inputs that meet the conditions the comparisons rest on, the observed data of the model-space cases, and the 80-bit
evaluation of the kernels of csrc/survey_misfit.hip with the bounds they are held to."""
import numpy as np

from zephyr_amd import misfit as mf

LD, CLD = np.longdouble, np.clongdouble
U64 = 2.0 ** -53
KINDS, SOURCES = mf.KINDS, mf.SOURCES
ALGEBRAIC = ('l2', 'huber', 'hybrid')
THRESHOLD, EPSILON = 0.2, 0.3
PARAMS = {'l2': {}, 'huber': dict(threshold=THRESHOLD), 'hybrid': dict(epsilon=EPSILON), 'logarithmic': dict(amplitude=1.0, phase=0.7)}
CODES = {'l2': 0, 'huber': 1, 'hybrid': 2, 'logarithmic': 3}
TAYLOR = 3.5          # the project's threshold: the error of a central difference falls by at least this per halving


def kernel_par(kind):
    'par0, par1 as the entry points take them'
    pr = PARAMS[kind]
    return {'l2': (0., 0.), 'huber': (pr.get('threshold', 0.), 0.), 'hybrid': (pr.get('epsilon', 0.), 0.),
            'logarithmic': (pr.get('amplitude', 0.), pr.get('phase', 0.))}[kind]


def randc(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- data-space inputs ----------------------------------------------------------------------------------------------------------------------------
# Built, not drawn and filtered: |p| and |s| in [1, 2], any phase; the residual r = q - d has sqrt(w2) |r| = t u with u from two bands, [0.2, 0.8] and
# [1.3, 3], so that both branches of 'huber' are present and no sample is within 0.2 t of the threshold; w2 in [0.5, 2] or absent.  Then |r| <= 0.85 <= 0.85 |q|:
# |q| / |d| lies in [0.54, 6.7] and |arg(q / d)| <= asin(0.85) < 1.02.  `conditions` verifies all of that on the 80-bit values.
BANDS = ((0.2, 0.8), (1.3, 3.0))


def panel_inputs(nrec, ncol, seed, weighted=True, dead=True):
    """p, d (nrec, ncol) complex128, w2 (nrec, ncol) float64 or None, s (ncol,) complex128.  dead: every seventh sample (and all of receiver 0 of column 0, when
    there is more than one receiver) has w2 = 0 and NaN in d"""
    rng = np.random.default_rng(seed)
    shape = (nrec, ncol)
    p = rng.uniform(1., 2., shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
    s = rng.uniform(1., 2., ncol) * np.exp(1j * rng.uniform(-np.pi, np.pi, ncol))
    w2 = rng.uniform(0.5, 2., shape) if weighted else None
    idx = np.arange(nrec * ncol).reshape(shape)
    band = np.where((idx + seed) % 2 == 0, 0, 1)
    lo = np.where(band == 0, BANDS[0][0], BANDS[1][0])
    hi = np.where(band == 0, BANDS[0][1], BANDS[1][1])
    u = lo + (hi - lo) * rng.uniform(0., 1., shape)
    r = THRESHOLD * u / np.sqrt(w2 if weighted else 1.) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
    d = s[None, :] * p - r
    if weighted and dead:
        off = idx % 7 == 3
        if nrec > 1:
            off[0, 0] = True
        w2 = np.where(off, 0., w2)
        d = np.where(off, complex(np.nan, np.nan), d)
    return p, d, w2, s


def conditions(p, d, w2, s):
    'the conditions on the inputs, on their 80-bit values: a dict of the figures the tests assert on'
    P, D, S = p.astype(CLD), d.astype(CLD), s.astype(CLD)
    live = np.ones(p.shape, dtype=bool) if w2 is None else w2 > 0
    W = np.ones(p.shape, dtype=LD) if w2 is None else w2.astype(LD)
    q = S[None, :] * P
    r = np.where(live, q - np.where(live, D, 1), 1)
    a = np.sqrt(np.where(live, W, 1)) * np.abs(r)
    rho = np.where(live, q / np.where(live, D, 1), 1)
    return dict(margin=float(np.min(np.abs(a[live] / LD(THRESHOLD) - 1))), below=int(np.count_nonzero(a[live] <= THRESHOLD)),
                above=int(np.count_nonzero(a[live] > THRESHOLD)), theta=float(np.max(np.abs(np.arctan2(rho.imag, rho.real)))),
                ratio=(float(np.min(np.abs(rho))), float(np.max(np.abs(rho)))), live=int(np.count_nonzero(live)), dead=int(np.count_nonzero(~live)))


def as3(x):
    'a panel (nrec, ncol) as the (nrec, nsrc, 1) data of one frequency; None stays None'
    return None if x is None else np.asarray(x)[:, :, None]


# ---- the kernels in 80-bit arithmetic, and what they are held to --------------------------------------------------------------------------------------
# Roundings per component, counted generously from the operation order of csrc/survey_misfit.hip (contraction is off there: a complex product is two
# products and a sum, 3 roundings; abs2 is 3).  With mu = |s|_1 |p|_1 + |d|_1 >= either component of q, d and r (|z|_1 = |Re z| + |Im z|):
#   moments:  w (conj(p) d) is 3 + 1, w |p|^2 is 3 + 1, each then summed over nrec                                   -> (nrec + 6) u  sum w |p|_1 |d|_1,  sum w |p|^2
#   r = s p - d carries at most 4 u mu per component.  psi = f r with f = w ('l2'), t sqrt(w) / |r| ('huber' beyond the threshold, where f < w and the
#   relative error of |r| is that of r, <= 4 sqrt(2) u mu / |r|, plus sqrt, product and quotient) or w / sqrt(1 + w |r|^2 / eps^2) ('hybrid', the same
#   argument with the factor x / (1 + x) <= 1): in every case below 24 u w mu                                          -> C_PSI u  w mu
#   phi per sample: |r|^2 within 20 u mu^2, then at most a square root, a quotient and three products, every branch below 64 u w mu^2; summed over nrec
#                                                                                                                    -> (nrec + 64) u  sum w mu^2
#   c = sum conj(psi) p: the error of psi times |p|_1, 3 for the product, nrec for the sum                           -> (nrec + C_PSI + 4) u  sum w mu |p|_1
#   v = phase (conj(s) psi + w (e d - f p)): 3 + 3 + 1 + 1 + 1 + 1 + 3                                               -> C_V u  |phase|_1 (|s|_1 |psi|_1 + w (|e|_1 |d|_1 + |f| |p|_1))
#   the Gauss-Newton weight W: |s|^2 w is 4; 'huber' and 'hybrid' add the relative error of |r|                       -> u W (8 + 8 mu / |r|)
C_PSI, C_V = 24, 14
def c_moments(nrec):
    return nrec + 6
def c_phi(nrec):
    return nrec + 64
def c_c(nrec):
    return nrec + C_PSI + 4
# 'logarithmic' runs through the device library's log and atan2, whose error cannot be counted from the code: the device is asked to lie within
# MARGIN max(delta, 64 u majorant) of the 80-bit value, delta what a numpy complex128 evaluation of the same formulas misses it by (the form of
# tests/krylov_cases.py), per column.  The majorants: per sample w (alpha (|L| + 1) + beta (|theta| + 1)) / |q| for psi -- an absolute error of a few u in L
# and theta is what a correctly rounded log and atan2 of an argument with a few u of relative error give --, its square form for phi and times |p|_1 for c.
MARGIN = 16.0


def l1(z):
    return np.abs(z.real) + np.abs(z.imag)


def reference(kind, p, d, w2, s, dtype=CLD):
    """mom (ncol, 3), psi (nrec, ncol), out (ncol, 3) = (phi_j, Re c_j, Im c_j) as the kernels define them, evaluated by zephyr_amd.misfit in `dtype`,
    and the majorants of the bounds above: dict(mom=(ncol, 3), psi=(nrec, ncol), out=(ncol, 3))"""
    real = LD if dtype is CLD else np.float64
    P, S = p.astype(dtype), s.astype(dtype)
    live = np.ones(p.shape, dtype=bool) if w2 is None else w2 > 0
    D = np.where(live, d, 1).astype(dtype)
    W = np.where(live, 1. if w2 is None else w2, 0).astype(real)
    a, b = mf.moments(as3(P), as3(D), as3(W), 'perSource')
    mom = np.stack([a[:, 0].real, a[:, 0].imag, b[:, 0]], axis=1)
    phi, psi, _ = mf._psi(as3(P), as3(D), S[:, None], as3(W), kind, PARAMS[kind])
    phi, psi = phi[:, :, 0], psi[:, :, 0]
    c = (np.conj(psi) * P).sum(axis=0)
    out = np.stack([phi.sum(axis=0), c.real, c.imag], axis=1)
    mu = l1(S)[None, :] * l1(P) + l1(D)
    maj = dict(mom=np.stack([(W * l1(P) * l1(D)).sum(axis=0)] * 2 + [(W * np.abs(P) ** 2).sum(axis=0)], axis=1))
    if kind == 'logarithmic':
        q = S[None, :] * P
        rho = q / D
        al, be = real(PARAMS[kind]['amplitude']), real(PARAMS[kind]['phase'])
        L, th = np.abs(np.log(np.abs(rho))), np.abs(np.arctan2(rho.imag, rho.real))
        mpsi = W * (al * (L + 1) + be * (th + 1)) / np.abs(q)
        mphi = W * (al * (L + 1) ** 2 + be * (th + 1) ** 2) / 2
    else:
        mpsi, mphi = W * mu, W * mu * mu
    mc = (mpsi * l1(P)).sum(axis=0)
    maj.update(psi=mpsi, out=np.stack([mphi.sum(axis=0), mc, mc], axis=1))
    return mom, psi, out, maj


def adjoint_reference(kind, psi, s, coef, p, d, w2, phase, dtype=CLD):
    'v (nrec, ncol), its majorant, the Gauss-Newton weights and the factor 8 + 8 mu / |r| of their bound (1 for the kinds without a residual in them)'
    real = LD if dtype is CLD else np.float64
    P, S, PSI = p.astype(dtype), s.astype(dtype), psi.astype(dtype)
    live = np.ones(p.shape, dtype=bool) if w2 is None else w2 > 0
    D = np.where(live, d, 1).astype(dtype)
    W = np.where(live, 1. if w2 is None else w2, 0).astype(real)
    v = np.conj(S)[None, :] * PSI
    mag = l1(S)[None, :] * l1(PSI)
    if coef is not None:
        e = (coef[:, 0] + 1j * coef[:, 1]).astype(dtype)
        f = coef[:, 2].astype(real)
        v = v + W * (e[None, :] * D - f[None, :] * P)
        mag = mag + W * (l1(e)[None, :] * l1(D) + np.abs(f)[None, :] * l1(P))
    if phase is not None:
        ph = phase.astype(dtype)
        v, mag = ph[:, None] * v, l1(ph)[:, None] * mag
    v = np.where(live, v, 0)
    pr = dict(PARAMS[kind])
    if kind == 'logarithmic':
        pr['phase'] = pr['amplitude']                      # (the weight panel exists for alpha = beta; the kernel reads par0 alone)
    gn = mf.gaussNewtonWeights(as3(P), as3(D), S[:, None], as3(W), kind, **pr)[:, :, 0]
    if kind in ('huber', 'hybrid'):
        r = S[None, :] * P - D
        factor = 8 + 8 * (l1(S)[None, :] * l1(P) + l1(D)) / np.where(live, np.abs(r), 1)
    else:
        factor = np.full(p.shape, 8.0)
    return v, mag, gn, factor


def worst(got, ref, bound):
    'max over components of |got - ref| / bound; where the bound is 0 the value must be exact'
    got = np.asarray(got)
    if np.iscomplexobj(ref):
        g = got.astype(CLD)
        err = np.maximum(np.abs(g.real - ref.real), np.abs(g.imag - ref.imag))
    else:
        err = np.abs(got.astype(LD) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max()) if ratio.size else 0.0


def held_ratio(err, held):
    'max of err / held, where a bound of zero asks for an exact value'
    err, held = np.asarray(err, dtype=LD), np.asarray(held, dtype=LD)
    ratio = np.where(held > 0, err / np.where(held > 0, held, 1), np.where(err > 0, np.inf, 0))
    return float(ratio.max()) if ratio.size else 0.0


def column_error(got, ref):
    'max over the rows of a panel, per column, of the componentwise error against the 80-bit value'
    g = np.asarray(got).astype(CLD if np.iscomplexobj(ref) else LD)
    err = np.maximum(np.abs(g.real - ref.real), np.abs(g.imag - ref.imag)) if np.iscomplexobj(ref) else np.abs(g - ref)
    return err.max(axis=0) if err.ndim == 2 else err


# ---- model space ------------------------------------------------------------------------------------------------------------------------------------
def observed(sv, dpred0, dpred1, seed=5, noise=0.02):
    'dobs of the model-space cases: the data of a perturbed model (dpred1), scaled by 1.3 - 0.4i, with 2 % noise (relative to the rms of the data) added'
    rng = np.random.default_rng(seed)
    shape = (sv.nrec, sv.nsrc, sv.nfreq)
    d = (1.3 - 0.4j) * np.asarray(dpred1).reshape(shape)
    rms = np.sqrt(np.mean(np.abs(d) ** 2, axis=(0, 1), keepdims=True))
    return d + noise * rms * randc(rng, shape) / np.sqrt(2.)


def central_ratios(f, g, c0, v, hs=(0.25, 0.125, 0.0625)):
    '|(f(c0 + h v) - f(c0 - h v)) / 2h - g . v| for h in hs, and the ratios of consecutive errors'
    dv = v.reshape(c0.shape)
    lin = float(np.dot(np.asarray(g).ravel(), v.ravel()))
    errs = [abs((f(c0 + h * dv) - f(c0 - h * dv)) / (2 * h) - lin) for h in hs]
    return errs, [errs[i] / errs[i + 1] for i in range(len(errs) - 1)], lin
