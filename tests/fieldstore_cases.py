"""Shared by tests/test_fieldstore.py (CPU) and tests/test_gpu_fieldstore.py (GPU): the columns the complex64 store is tested on, and the bound of its format."""
import numpy as np

NCOL = 13


def pack_columns(N, seed=0):
    """(N, 13) complex128: magnitudes from 1e-300 to 1e300; column 1 zero; column 2 with its largest component in its LAST element; column 0 with one element
    2^-140 of its largest (an fp32 subnormal after scaling, or flushed); a subnormal column (the exponent clamp); columns of mixed dynamic range."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((N, NCOL)) + 1j * rng.standard_normal((N, NCOL))
    mags = [1.0, 0.0, 3.0, 1e-300, 1e300, 1e-310, 1e-150, 1e150, 7e-39, 2.0 ** 127, 1e-5, 2.0 ** -126, 1e38]
    U *= np.array(mags)[None, :]
    U[:, 2] *= 0.25
    U[N - 1, 2] = 3.0 * (2.5 - 0.5j)                              # the column maximum is the last element's real part
    U[0, 0] = 4.0 + 0.125j                                        # the column maximum, pinned: the rest of the column is clipped below it
    U[1:, 0] = np.clip(U[1:, 0].real, -3.5, 3.5) + 1j * np.clip(U[1:, 0].imag, -3.5, 3.5)
    if N > 1:
        U[N // 2, 0] = 4.0 * 2.0 ** -140 * (1 - 1j)
    U[:, 10] *= 10.0 ** rng.uniform(-30, 0, N)                    # thirty decades inside one column
    return U


def pack_bound_violations(U, V, e):
    """per component of the unpacked V against the fp64 input U, with thr_s = 2^(e_s - 126): |V - U| <= 2^-24 |U| where |U| >= thr_s (the scaled value is a
    normal fp32 number: half an ulp), |V - U| <= thr_s below (an fp32 subnormal, or flushed).  Returns the number of components outside.  Extended precision
    only to REPRESENT the thresholds (2^-1147 is below fp64's range); the comparison itself is exact."""
    ld = np.longdouble
    U = np.asarray(U).reshape((np.asarray(U).shape[0], -1))
    V = np.asarray(V).reshape(U.shape)
    thr = np.ldexp(ld(1), np.asarray(e, dtype=np.int64) - 126)[None, :]
    bad = 0
    for x, y in ((U.real, V.real), (U.imag, V.imag)):
        ok = np.isfinite(y)
        ax = np.abs(x.astype(ld))
        err = np.abs(y.astype(ld) - x.astype(ld))
        lim = np.where(ax >= thr, ld(2.0) ** -24 * ax, thr)
        bad += int(np.count_nonzero(~ok | ~(err <= lim)))
    return bad
