"""Shared by tests/test_illumination_host.py (CPU) and tests/test_gpu_illumination.py (GPU): the columns the energy kernels are tested on, their
extended-precision evaluation, the bound derived from the arithmetic, and deliberately wrong evaluations the bound has to catch.

The kernels compute, per cell i,  E[i] += alpha * W[i] * sum_{s<nsrc} (Re u_s[i]^2 + Im u_s[i]^2)  in plain fp64 with the sum over s in the order
s = 0, 1, ...  Every term is non-negative, so every rounding multiplies a partial result by (1 + d), |d| <= u = 2^-53, and the errors never cancel
against anything: the bound is componentwise and relative.  Counting the factors the most-rounded term collects:

    |u_s|^2 = fl(fl(re^2) + fl(im^2))        2   (each square once, the addition once: (a (1+d1) + b (1+d2)) (1+d3) lies within (1+u)^2 of a + b)
    sum over s, in order                     nsrc - 1   (the first term goes through every addition)
    alpha * W, its product with the sum      2
    the addition to E                        1

(1 + u)^(nsrc + 4) - 1 <= (nsrc + 7) u for every nsrc below 2^40.  A contraction (fma) removes a rounding and never adds one.  Successive launches onto the
same E multiply their factors, so their bounds add (to first order; the slack of 3 u per launch covers the rest).  The squares must neither overflow nor
go subnormal for this to hold, which is why the columns stay between 1e-140 and 1e140.
"""
import numpy as np

U_RND = 2.0 ** -53
NPATTERN = 13
LD = np.longdouble
# column j of energy_columns is of kind PATTERN[j % 13]
PATTERN = [1.0, 'zero', 'last', 1e-140, 1e140, 'decades', 1e-70, 1e70, 3.0, 1e-3, 0.5, 2.0 ** -100, 2.0]


def energy_columns(N, cols, seed=0):
    """(N, len(cols)) complex128, column k of kind PATTERN[cols[k] % 13]: moduli in [0.5, 2) times the kind's magnitude with uniform phases; 'zero' a zero
    column; 'last' a column whose only nonzero is its last element; 'decades' thirty decades inside one column."""
    cols = list(cols)
    rng = np.random.default_rng(seed)
    U = (0.5 + 1.5 * rng.random((N, len(cols)))) * np.exp(2j * np.pi * rng.random((N, len(cols))))
    for k, j in enumerate(cols):
        kind = PATTERN[j % NPATTERN]
        if kind == 'zero':
            U[:, k] = 0.0
        elif kind == 'last':
            U[:-1, k] = 0.0
            U[-1, k] = 3.0 * (2.5 - 0.5j)
        elif kind == 'decades':
            U[:, k] *= 10.0 ** rng.uniform(-30, 0, N)
        else:
            U[:, k] *= kind
    return U


def energy_exact(U, alpha=1.0, W=None, E0=None):
    'E0 + alpha W sum_s |u_s|^2 per cell in 80-bit arithmetic (np.longdouble) from the fp64 values given: (N,) longdouble'
    U = np.asarray(U).reshape((np.asarray(U).shape[0], -1))
    s = (U.real.astype(LD) ** 2 + U.imag.astype(LD) ** 2).sum(axis=1)
    w = LD(alpha) * (LD(1) if W is None else np.asarray(W).astype(LD))
    return (LD(0) if E0 is None else np.asarray(E0).astype(LD)) + w * s


def energy_bound(exact, nsrc):
    """(nsrc + 7) 2^-53 exact per launch (the module docstring derives it): `nsrc` the columns of one launch, or a sequence with those of every launch that
    added to the result; `exact` the extended-precision value of the final result"""
    n = sum(int(k) + 7 for k in np.atleast_1d(nsrc))
    return LD(n) * LD(U_RND) * np.asarray(exact).astype(LD)


def energy_check(got, exact, nsrc, extra=0.0):
    """(violations, worst |got - exact| / bound): the cells of `got` (fp64) outside energy_bound (+ extra * u * exact, for callers whose weights carry
    roundings of their own), non-finite ones included, and the largest error ratio among the cells with a positive bound (0.0: every error is zero)"""
    got = np.asarray(got, dtype=np.float64)
    exact = np.asarray(exact).astype(LD)
    bound = energy_bound(exact, nsrc) + LD(extra) * LD(U_RND) * exact
    err = np.abs(got.astype(LD) - exact)
    bad = ~np.isfinite(got) | ~(err <= bound)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return int(np.count_nonzero(bad)), worst


def energy_fp64(U, alpha=1.0, W=None, E0=None):
    "the kernels' arithmetic in numpy: plain fp64, the sum over s in order"
    U = np.asarray(U).reshape((np.asarray(U).shape[0], -1))
    acc = np.zeros(U.shape[0])
    for s in range(U.shape[1]):
        acc = acc + (U[:, s].real * U[:, s].real + U[:, s].imag * U[:, s].imag)
    w = alpha if W is None else alpha * np.asarray(W, dtype=np.float64)
    return (0.0 if E0 is None else np.asarray(E0, dtype=np.float64)) + w * acc


def energy_wrong(U, how, alpha=1.0, W=None, E0=None, col=0):
    "a deliberately wrong evaluation: how = 'real_only' squares only the real part of column `col`, 'skip_last' leaves the last column out"
    U = np.array(np.asarray(U).reshape((np.asarray(U).shape[0], -1)))
    if how == 'real_only':
        U[:, col] = U[:, col].real
    elif how == 'skip_last':
        U = U[:, :-1]
    else:
        raise ValueError(how)
    return energy_fp64(U, alpha, W, E0)


def energy_entry(rng, exact_add):
    """a non-negative E on entry that matters next to what a launch adds (`exact_add`, (N,)): a third of the cells zero, the others between 0.1 and 10 times the
    addition (1.0 where the addition is zero)"""
    add = np.asarray(exact_add).astype(np.float64)
    E0 = np.where(add > 0, add, 1.0) * 10.0 ** rng.uniform(-1, 1, add.shape)
    E0[rng.random(add.shape) < 1.0 / 3] = 0.0
    return E0
